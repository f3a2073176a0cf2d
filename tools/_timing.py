"""Device-event timing, as the bench tools under tools/ report it."""
import numpy as np
import torch


def timed(fn, warmup, reps, inner):
    """`warmup` calls of `fn`, then `reps` windows of `inner` back-to-back calls between two events on the current stream
    -> median, min and max of the per-call time in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record(); b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": reps, "inner": inner}
