"""Host helpers shared by the evaluation wrappers (postprocess.py, detection_ap.py, caption_eval.py, predictions.py)."""
import numpy as np
import torch

MAX_PROPOSALS = 512   # K of the one-thread-per-proposal kernels (csrc/postprocess.hip, detection_ap.hip, predictions.hip)

_NUMPY = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64,
          torch.float32: np.float32, torch.float64: np.float64}


def gpu(prefix, t, name):
    """``t`` when it is a device tensor; there is no host fallback."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{prefix}: {name}: CPU not supported")
    return t


def mask_u8(t):
    """A bool or number mask as the contiguous uint8 (0 / 1) the kernels read."""
    return t.contiguous().view(torch.uint8) if t.dtype == torch.bool else (t != 0).to(torch.uint8)


def ptr(t):
    return None if t is None else t.data_ptr()


def word(idx2word, i):
    """``idx2word`` maps ``str(id)`` (the reference's vocabulary) or the int id to the word."""
    try:
        return idx2word[str(i)]
    except (KeyError, TypeError, IndexError):
        return idx2word[i]


def to_host(tensors):
    """A list or dict of device tensors as numpy arrays of the same dtypes and shapes (a list or dict alike), by ONE
    device-to-host copy: the tensors travel concatenated as bytes."""
    parts = [t.contiguous() for t in (tensors.values() if isinstance(tensors, dict) else tensors)]
    flat = torch.cat([p.reshape(-1).view(torch.uint8) for p in parts]).cpu().numpy()
    host, off = [], 0
    for p in parts:
        nb = p.numel() * p.element_size()
        host.append(flat[off:off + nb].view(_NUMPY[p.dtype]).reshape(tuple(p.shape)))
        off += nb
    return dict(zip(tensors, host)) if isinstance(tensors, dict) else host
