"""Caption decoding over the kept proposals only (csrc/decode_select.hip): the pieces that make the
decoder's rows sparse.  Every reader of ``lang_cap`` reads it only where post-processing kept the box, and the decoders of
``caption_decode`` take any number of independent rows, so:

* ``select``         -- the flagged (scene, proposal) pairs as a dense row list, in flat order;
* ``gather``         -- the decoder's indicator rows read through that list (padding rows are zero);
* ``scatter_words``  -- the decoded words back at their proposals, the empty caption elsewhere;
* ``scatter_values`` -- the same for scores and lengths, with a scalar fill.

One launch each on the current stream, no host synchronisation (capturable in a graph), every element of every output
written.  CPU tensors raise ``RuntimeError("... CPU not supported")``: there is no host fallback.
"""
import torch

from ._eval_util import gpu, mask_u8
from ._native import check, lib

MAX_FLAGS = 65536     # n of spacap_decode_select_i32: one workgroup ranks them


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _index(name, t, dev):
    gpu("decode_select", t, name)
    if t.dtype != torch.int32 or t.dim() != 1 or t.device != dev:
        raise RuntimeError(f"decode_select: {name} must be an int32 vector on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t.contiguous()


def select(mask, capacity):
    """``mask``: bool or number flags of any shape (B, K), n = B K <= 65 536 of them; any non-zero value is set.  ``capacity``:
    the length of the row list, 1..n.  Returns ``(rows, slot, count)``: ``rows`` int32 (capacity,) the flat indices of the
    first ``capacity`` set flags in flat order, -1 behind the last; ``slot`` int32 (n,) the position of every flag in ``rows``,
    -1 where the flag is clear or did not fit; ``count`` int32 (2,) = the number of set flags and min(that, capacity)."""
    mask = gpu("decode_select", mask, "mask")
    n = mask.numel()
    if not 1 <= n <= MAX_FLAGS:
        raise RuntimeError(f"decode_select: mask has {n} flags, supported 1..{MAX_FLAGS}")
    capacity = int(capacity)
    if not 1 <= capacity <= n:
        raise ValueError(f"decode_select: capacity {capacity} outside 1..{n}")
    dev = mask.device
    m = mask_u8(mask).reshape(-1)
    with torch.cuda.device(dev):
        rows = torch.empty(capacity, dtype=torch.int32, device=dev)
        slot = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        check(lib.spacap_decode_select_i32(m.data_ptr(), n, capacity, rows.data_ptr(), slot.data_ptr(), count.data_ptr(), _stream(dev)),
              "spacap_decode_select_i32")
    return rows, slot, count


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def gather(obj, memory, rows):
    """``obj`` f32 (n, d), ``memory`` f32 (n, d) or None, ``rows`` int32 (capacity,) from ``select``; d a multiple of 4.
    Returns f32 (capacity, d): ``obj[rows[i]] + memory[rows[i]]`` (``obj[rows[i]]`` alone without ``memory``), zeros where
    ``rows[i]`` < 0 -- the sum is formed for the packed rows only."""
    obj = gpu("decode_select", obj, "obj")
    dev = obj.device
    if obj.dim() != 2 or obj.dtype != torch.float32 or obj.shape[1] % 4 or obj.shape[1] < 4:
        raise RuntimeError(f"decode_select: obj must be float32 (n, d) with d a multiple of 4, got {tuple(obj.shape)} {obj.dtype}")
    if memory is not None:
        gpu("decode_select", memory, "memory")
        if memory.shape != obj.shape or memory.dtype != torch.float32 or memory.device != dev:
            raise RuntimeError(f"decode_select: memory must be float32 {tuple(obj.shape)} on {dev}, got {tuple(memory.shape)} "
                               f"{memory.dtype} on {memory.device}")
        memory = _aligned(memory.contiguous())
    rows = _index("rows", rows, dev)
    obj = _aligned(obj.contiguous())
    cap, d = rows.shape[0], obj.shape[1]
    with torch.cuda.device(dev):
        out = torch.empty(cap, d, dtype=torch.float32, device=dev)
        check(lib.spacap_decode_gather_f32(obj.data_ptr(), None if memory is None else memory.data_ptr(), rows.data_ptr(), cap, d,
                                           out.data_ptr(), _stream(dev)), "spacap_decode_gather_f32")
    return out


def _inner(name, t, slot):
    if t.dim() < 1 or t.shape[0] < 1:
        raise RuntimeError(f"decode_select: {name} must hold one row or more, got {tuple(t.shape)}")
    if t.device != slot.device:
        raise RuntimeError(f"decode_select: {name} must be on {slot.device}")
    inner = t[0].numel()
    if inner < 1:
        raise RuntimeError(f"decode_select: {name} has empty rows, got {tuple(t.shape)}")
    return inner


def scatter_words(ys, slot, eos):
    """``ys`` int64 (capacity, ..., L) words of the packed rows, ``slot`` int32 (n,) from ``select``.  Returns int64
    (n, ..., L): row j is ``ys[slot[j]]`` where ``slot[j]`` >= 0 and elsewhere the empty caption, once per L words:
    ``eos`` followed by zeros."""
    ys = gpu("decode_select", ys, "ys")
    slot = _index("slot", slot, ys.device)
    if ys.dtype != torch.int64 or ys.dim() < 2:
        raise RuntimeError(f"decode_select: ys must be int64 (capacity, ..., L), got {tuple(ys.shape)} {ys.dtype}")
    inner, L, n, dev = _inner("ys", ys, slot), ys.shape[-1], slot.shape[0], ys.device
    ys = ys.contiguous()
    with torch.cuda.device(dev):
        out = torch.empty((n,) + tuple(ys.shape[1:]), dtype=torch.int64, device=dev)
        check(lib.spacap_decode_scatter_i64(ys.data_ptr(), slot.data_ptr(), n, inner, L, int(eos), out.data_ptr(), _stream(dev)),
              "spacap_decode_scatter_i64")
    return out


def scatter_values(vals, slot, fill):
    """``vals`` float32 or int32 (capacity, ...) values of the packed rows, ``slot`` int32 (n,) from ``select``.  Returns
    (n, ...) of the same dtype: row j is ``vals[slot[j]]`` where ``slot[j]`` >= 0 and ``fill`` elsewhere."""
    vals = gpu("decode_select", vals, "vals")
    slot = _index("slot", slot, vals.device)
    if vals.dtype not in (torch.float32, torch.int32):
        raise RuntimeError(f"decode_select: vals must be float32 or int32, got {vals.dtype}")
    inner, n, dev = _inner("vals", vals, slot), slot.shape[0], vals.device
    vals = vals.contiguous()
    with torch.cuda.device(dev):
        out = torch.empty((n,) + tuple(vals.shape[1:]), dtype=vals.dtype, device=dev)
        if vals.dtype == torch.float32:
            check(lib.spacap_decode_scatter_f32(vals.data_ptr(), slot.data_ptr(), n, inner, float(fill), out.data_ptr(), _stream(dev)),
                  "spacap_decode_scatter_f32")
        else:
            check(lib.spacap_decode_scatter_i32(vals.data_ptr(), slot.data_ptr(), n, inner, int(fill), out.data_ptr(), _stream(dev)),
                  "spacap_decode_scatter_i32")
    return out
