"""The two-rank reference of the data-parallel AdamW step (co_occ_amd/optim.py): rank ``r`` draws its gradients with
``optim_refs.gradients(cs, seed=r)``, the ranks' average ``g0/2 + g1/2`` is taken in fp32 on the CPU -- with two ranks the sum is
one rounding and does not depend on the order -- and ``optim_refs.run`` steps the case set on it in float64 (the judge) and float32
(the anchor).  No GPU here; computed once per process and shared."""
import torch

import optim_refs as R

WORLD = 2
_CACHE = {}


def rank_gradients(cs, rank):
    return R.gradients(cs, seed=rank)


def average(rows_per_rank):
    """[step][case] of the fp32 average over the ranks' rows, None where the ranks have none."""
    out = []
    for rows in zip(*rows_per_rank):
        row = []
        for gs in zip(*rows):
            if gs[0] is None:
                row.append(None)
            else:
                acc = gs[0] / len(gs)
                for g in gs[1:]:
                    acc = acc + g / len(gs)
                row.append(acc)
        out.append(row)
    return out


def averaged_reference(chunk, max_norm=R.MAX_NORM):
    """(case list, p0, averaged gradient rows, float64 run, float32 run) for two ranks."""
    key = (chunk, max_norm)
    if key not in _CACHE:
        cs = R.cases(chunk)
        p0 = R.initial(cs, 0)
        rows = average([rank_gradients(cs, r) for r in range(WORLD)])
        _CACHE[key] = (cs, p0, rows, R.run(cs, p0, rows, max_norm, torch.float64), R.run(cs, p0, rows, max_norm, torch.float32))
    return _CACHE[key]
