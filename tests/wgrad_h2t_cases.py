"""Rule books for the tests of ``coocc_conv_wgrad_h2t`` (csrc/wgrad_h2t.hip): a random row table with the cases the kernel's
skip branch and range-checked loads have to get right, and the gathered operand of one tap for the float64 restatement."""
import numpy as np
import torch

LIVE = 0.3           # share of live entries outside the dead tap and the dead run


def dead_tap(taps):
    """The tap whose every entry is -1 (none when the book has one tap)."""
    return taps // 2 if taps > 1 else None


def dead_run(M):
    """(start, stop) of the aligned 16-row run that is -1 for every tap (None below 32 rows: it would leave next to nothing)."""
    if M < 32:
        return None
    start = (M // 32) * 16
    return start, start + 16


def book(taps, M, in_rows, seed):
    """int32 [taps, M] with about ``LIVE`` of the entries a row of [0, in_rows) and the rest -1; tap ``dead_tap(taps)`` all -1;
    rows ``dead_run(M)`` -1 for every tap; every other tap has at least one live entry."""
    g = np.random.default_rng(seed)
    tb = g.integers(0, in_rows, size=(taps, M)).astype(np.int32)
    tb[g.random((taps, M)) >= LIVE] = -1
    run = dead_run(M)
    rows = [m for m in range(M) if run is None or not run[0] <= m < run[1]]
    for t in range(taps):                       # one forced live entry per tap, outside the dead run
        tb[t, rows[(7 * t) % len(rows)]] = (13 * t + 5) % in_rows
    if run is not None:
        tb[:, run[0]:run[1]] = -1
    if dead_tap(taps) is not None:
        tb[dead_tap(taps)] = -1
    return tb


def gathered(x, tb_t):
    """Rows of ``x`` [in_rows, C] (torch, CPU) read through one tap's ids [M] (numpy): zeros where the book holds -1."""
    idx = torch.from_numpy(np.maximum(tb_t, 0).astype(np.int64))
    return x[idx] * torch.from_numpy((tb_t >= 0)).to(x.dtype)[:, None]
