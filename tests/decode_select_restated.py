"""Numpy restatement of csrc/decode_select.hip, written as plain loops: it is the specification the
kernels and the masked ``forward_eval`` are held to (tests/test_decode_select_cpu.py, tests/test_decode_select_gpu.py)."""
import numpy as np

SIZES = (1, 63, 64, 65, 255, 256, 257, 2048, 2049, 65536)      # n: around a wave, the workgroup, the chunk length, the limit
DENSITIES = (0.0, 0.1, 0.5, 1.0)


def select(mask, capacity):
    """mask: n flags (any non-zero value is set), capacity in 1..n -> rows i32 (capacity,), slot i32 (n,), count i32 (2,)."""
    mask = np.asarray(mask).reshape(-1)
    n = mask.shape[0]
    assert 1 <= capacity <= n
    rows = np.full(capacity, -1, np.int32)
    slot = np.full(n, -1, np.int32)
    seen = 0
    for j in range(n):
        if mask[j] != 0:
            if seen < capacity:
                rows[seen] = j
                slot[j] = seen
            seen += 1
    return rows, slot, np.array([seen, min(seen, capacity)], np.int32)


def gather(obj, memory, rows):
    """obj, memory (or None) f32 (n, d), rows i32 (capacity,) -> f32 (capacity, d); a padding row is +0.0."""
    out = np.zeros((rows.shape[0], obj.shape[1]), np.float32)
    for i in range(rows.shape[0]):
        if rows[i] >= 0:
            out[i] = obj[rows[i]] if memory is None else obj[rows[i]] + memory[rows[i]]
    return out


def scatter_words(ys, slot, L, eos):
    """ys i64 (capacity, inner), slot i32 (n,), inner a multiple of L -> i64 (n, inner); no slot: the empty caption repeated."""
    inner = ys.shape[1]
    assert inner % L == 0
    out = np.empty((slot.shape[0], inner), np.int64)
    for j in range(slot.shape[0]):
        if slot[j] >= 0:
            out[j] = ys[slot[j]]
        else:
            for l in range(inner):
                out[j, l] = eos if l % L == 0 else 0
    return out


def scatter_values(vals, slot, fill):
    """vals (capacity, inner) f32 or i32, slot i32 (n,) -> (n, inner) of the same dtype; no slot: fill."""
    out = np.empty((slot.shape[0], vals.shape[1]), vals.dtype)
    for j in range(slot.shape[0]):
        if slot[j] >= 0:
            out[j] = vals[slot[j]]
        else:
            for l in range(vals.shape[1]):
                out[j, l] = fill
    return out


def capacities(n, count):
    """The capacities of the tests: 1, count - 1, count, count + 1 and n, clipped to 1..n, each once."""
    return sorted({min(max(c, 1), n) for c in (1, count - 1, count, count + 1, n)})


_MASKS, _SELECTED = {}, {}


def select_case(n, density, capacity):
    """``select`` of ``mask_case(n, density)``, computed once and shared (read-only)."""
    key = (n, density, capacity)
    if key not in _SELECTED:
        _SELECTED[key] = select(mask_case(n, density), capacity)
        for a in _SELECTED[key]:
            a.setflags(write=False)
    return _SELECTED[key]


def mask_case(n, density):
    """The flags of one case, computed once and shared (read-only): density 0 / 1 are all clear / all set; set bytes take
    values other than 1 as well."""
    key = (n, density)
    if key not in _MASKS:
        rng = np.random.default_rng(1000 * n + int(density * 100))
        m = (rng.random(n) < density).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
        m.setflags(write=False)
        _MASKS[key] = m
    return _MASKS[key]
