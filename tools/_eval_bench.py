"""What the timing tools of the evaluation operators share (bench_postprocess.py, bench_detection_ap.py,
bench_caption_eval.py, bench_predictions.py): device time by graph replay, the time of one eager call, and the steps that
make a checkout of the reference importable on the CPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def replay_us(fn, iters, settle=0):
    """Device time of ``fn()`` in microseconds: warmed up on a side stream, captured in a graph, replayed ``settle`` times
    untimed and then ``iters`` times back to back between two HIP events (no host work in between), five times over; the
    median.  Also returns what ``fn`` returned under capture (the graph's static outputs)."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    for _ in range(settle):
        g.replay()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(5):
        t0.record()
        for _ in range(iters):
            g.replay()
        t1.record()
        t1.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / iters)
    return float(np.median(us)), out


def eager_us(fn, iters, before=None):
    """Median time of one eager ``fn()`` in microseconds between two HIP events on an idle device: the Python wrapper's host
    work is included.  ``before()`` runs ahead of every call, untimed."""
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(iters):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3)
    return float(np.median(us))


def enter_reference(ref_dir):
    """Makes the reference checkout ``ref_dir`` importable in this process (no GPU needed): stand-ins for the modules it
    imports and does not use here, its directory as the working directory and on ``sys.path``.  Returns the fixture module
    (tests/golden/make_fixtures_postprocess.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_fixtures_postprocess as fixtures
    fixtures.install_stubs()
    os.chdir(ref_dir)
    sys.path.insert(0, ref_dir)
    return fixtures
