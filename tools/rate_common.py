"""What the *_rate.py tools share (they run as scripts, so this imports as `rate_common`): HIP-event timing of a body, the bracket around
the library's kernel timing kinds, and the JSON-lines record writer."""
import contextlib
import json
import os
import types

import numpy as np


def timed(torch, stream, body, reps, warmup):
    """Mean milliseconds of body() between HIP events recorded on `stream`, after `warmup` untimed calls."""
    for _ in range(warmup):
        body()
    torch.cuda.synchronize()
    start = [torch.cuda.Event(enable_timing=True) for _ in range(reps)]
    stop = [torch.cuda.Event(enable_timing=True) for _ in range(reps)]
    with torch.cuda.stream(stream):
        for i in range(reps):
            start[i].record(stream)
            body()
            stop[i].record(stream)
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in zip(start, stop)]))


@contextlib.contextmanager
def kernel_timing(ctx, kind):
    """`with kernel_timing(ctx, kind) as t:` times the launches of kernel timing kind `kind` made in the block; afterwards t.ms is their
    total milliseconds and t.launches their number."""
    t = types.SimpleNamespace()
    ctx.kernel_time(kind, reset=True)
    ctx.set_kernel_timing([kind])
    yield t
    ctx.synchronize()
    ctx.set_kernel_timing(False)
    t.ms, t.launches = ctx.kernel_time(kind, reset=True)


class Records:
    """emit(rec): the record plus the fields every record of the run carries, as one JSON line on stdout and, with `path`, in that file."""

    def __init__(self, path, **common):
        self.common = common
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.out = open(path, "w") if path else None

    def emit(self, rec):
        line = json.dumps(dict(rec, **self.common))
        print(line, flush=True)
        if self.out:
            self.out.write(line + "\n")
            self.out.flush()
