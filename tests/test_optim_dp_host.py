"""Data-parallel gradient averaging, host half (no GPU; co_occ_amd/optim.py): the arena layout and the fingerprint
are functions of the shapes alone, ``process_group=None`` is the optimizer it was, the new entries are declared, bound and
validate before they launch, what is refused is refused by name -- and the two-rank reference the GPU tests step has both clip
regimes."""
import ctypes

import numpy as np
import pytest
import torch

from co_occ_amd import _lib, optim

import optim_refs as R
import optim_dp_refs as D
import test_abi

ENTRY_POINTS = ("coocc_optim_pack", "coocc_optim_unpack", "coocc_optim_flag_check")
one = ctypes.c_void_p(256)          # a non-null 16-byte aligned dummy address: validation never dereferences device pointers


def _numels(chunk):
    return [R.numel(shape) for _, shape, kind in R.cases(chunk) if kind != "frozen"]


# ----------------------------------------------------------------------------- the reference the GPU tests rely on
def test_both_clip_regimes_occur_in_the_two_rank_average():
    chunk = optim.chunk_size()
    cs, p0, rows, r64, r32 = D.averaged_reference(chunk)
    n = r64["norms"]
    print("[optim-dp] float64 norms of the two-rank average:", n)
    assert len(n) == 4 and n[0] < R.MAX_NORM / 2 and n[2] < R.MAX_NORM / 2 and n[1] > 2 * R.MAX_NORM and n[3] > 2 * R.MAX_NORM, n
    # with two ranks a/2 + b/2 is one rounding: the same bits as (a + b)/2, whatever the order
    ga, gb = R.gradients(cs, seed=0), R.gradients(cs, seed=1)
    for ra, rb, row in zip(ga, gb, rows):
        for a, b, avg in zip(ra, rb, row):
            assert (a is None) == (b is None) == (avg is None)
            if a is not None:
                assert avg.numpy().tobytes() == ((a + b) / 2).numpy().tobytes() == (b / 2 + a / 2).numpy().tobytes()
    # and the averaged run is not rank 0's own run: a test that compares against it can tell the two apart
    own = R.reference(chunk)[3]
    far = max(float((x - y).abs().max()) for x, y in zip(r64["p"], own["p"]) if x.numel())
    assert far > 1e-2, far


# ----------------------------------------------------------------------------- the layout
def test_layout_offsets_are_aligned_ascending_and_disjoint():
    chunk = optim.chunk_size()
    numels = [R.numel(shape) for _, shape, _ in R.cases(chunk)]          # the empty tensor included
    lay = optim.arena_layout(numels)
    live = [i for i, n in enumerate(numels) if n > 0]
    assert lay.numels == tuple(numels) and lay.header == len(live) == len(numels) - 1, "one header float per tensor with elements"
    assert lay.offsets.dtype == np.int64 and lay.offsets[numels.index(0)] == -1, "an empty tensor gets no segment"
    end = lay.header
    for i in live:
        o = int(lay.offsets[i])
        assert o % 4 == 0 and o >= end, "segment %d at %d: a multiple of 4 behind the previous segment's end %d" % (i, o, end)
        assert o - end < 4 or end == lay.header, "no more padding than the alignment needs"
        end = o + numels[i]
    assert lay.total >= end and lay.total % 4 == 0 and lay.total - end < 4
    assert int(lay.offsets[live[0]]) == (lay.header + 3) // 4 * 4
    assert optim.arena_layout([]).total == 0 and optim.arena_layout([0, 0]).header == 0
    assert optim.arena_layout([1]).offsets.tolist() == [4] and optim.arena_layout([1]).total == 8
    assert optim.arena_layout([5, 4, 3]).offsets.tolist() == [4, 12, 16] and optim.arena_layout([5, 4, 3]).total == 20
    with pytest.raises(ValueError, match="negative"):
        optim.arena_layout([3, -1])


def test_layout_and_fingerprint_depend_on_the_shapes_alone():
    chunk = optim.chunk_size()
    a = [torch.zeros(n) for n in _numels(chunk)]
    b = [torch.randn(n) for n in _numels(chunk)]                       # other values, other addresses, same shapes
    la, lb = optim.arena_layout([t.numel() for t in a]), optim.arena_layout([t.numel() for t in b])
    assert la.header == lb.header and la.total == lb.total and np.array_equal(la.offsets, lb.offsets)
    fa = optim.fingerprint([t.numel() for t in a])
    assert fa == optim.fingerprint([t.numel() for t in b])
    assert len(fa) == 3 and all(isinstance(v, int) and 0 <= v < 2 ** 62 for v in fa), "three values that an int64 sum of one row keeps"
    assert fa[0] == len(a) and fa[1] == sum(t.numel() for t in a)


def test_fingerprint_differs_when_a_numel_or_the_count_differs():
    base = _numels(optim.chunk_size())
    f = optim.fingerprint(base)
    assert optim.fingerprint(base + [10]) != f and optim.fingerprint(base[:-1]) != f
    moved = list(base)
    moved[0], moved[1] = moved[0] + 1, moved[1] - 1                    # same count, same total: only the hash tells
    g = optim.fingerprint(moved)
    assert g[:2] == f[:2] and g[2] != f[2]
    swapped = list(base)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    assert swapped != base and optim.fingerprint(swapped)[:2] == f[:2] and optim.fingerprint(swapped)[2] != f[2], "the order counts"


# ----------------------------------------------------------------------------- the optimizer without a group
def test_process_group_none_constructs_and_behaves_as_before():
    ps = [torch.nn.Parameter(torch.randn(s)) for s in ((5,), (3, 4))]
    opt = optim.AdamW(R.make_groups(ps), max_grad_norm=5)
    assert opt.process_group is None and opt.dp_always is False and opt.write_reduced_grad is False
    assert opt.grad_mismatch is None
    opt.release_arena()                                              # nothing to release: no error
    assert opt._dp_mode() is None, "no group, no dp_always: the single-rank path"
    sd = opt.state_dict()
    assert "process_group" not in sd["param_groups"][0], "the group is no hyper-parameter: checkpoints stay torch's"
    assert sd["param_groups"][0].keys() == torch.optim.AdamW(R.make_groups(ps)).state_dict()["param_groups"][0].keys()
    ps[1].grad = torch.ones_like(ps[1])
    with pytest.raises(ValueError, match=r"parameter 1 .*HIP device"):          # the refusal of the path it always took
        opt.step()
    assert len(opt.state) == 0
    for pg in (True, "world"):
        assert optim.AdamW(ps, process_group=pg).process_group == pg       # resolved at the first step, not here


def test_refusal_texts():
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3))]
    for bad in (1, "all", 2.5, object()):
        with pytest.raises(ValueError, match="process_group="):
            optim.AdamW(ps, process_group=bad)
    with pytest.raises(ValueError, match="process_group="):
        optim.all_reduce_gradients(ps, group="ranks")
    with pytest.raises(ValueError, match="process_group="):
        optim.broadcast_parameters(ps, group=3)
    assert not torch.distributed.is_initialized()
    opt = optim.AdamW(ps, process_group=True)
    ps[0].grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="AdamW: .*not initialised"):
        opt.step()
    assert len(opt.state) == 0, "a refused step changes nothing"
    with pytest.raises(RuntimeError, match="all_reduce_gradients: .*not initialised"):
        optim.all_reduce_gradients(ps)
    with pytest.raises(RuntimeError, match="broadcast_parameters: .*not initialised"):
        optim.broadcast_parameters(ps)
    # the arena path names the parameter, in _check_param's words
    opt = optim.AdamW(ps)
    opt.dp_always = True
    with pytest.raises(ValueError, match=r"parameter 0 .*HIP device"):
        opt.step()
    assert len(opt.state) == 0
    frozen = torch.nn.Parameter(torch.randn(4), requires_grad=False)
    frozen.grad = torch.ones(4)
    opt = optim.AdamW([ps[1], frozen])
    opt.dp_always = True
    ps[1].grad = None
    with pytest.raises(ValueError, match=r"parameter 1 .*requires_grad=False"):
        opt._layout_reducer()


# ----------------------------------------------------------------------------- ABI
def test_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fns = test_abi.header_functions()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), "missing export " + name
        assert name in fns, name + " is not declared in include/coocc_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == fns[name], name


def test_entry_points_validate_before_launching():
    """COOCC_EINVAL (-1) with the entry's own name before any launch (so without a GPU): null tables, a chunk count that is not the
    table's, an arena that is null or misaligned, segments that are misaligned, outside the arena, overlapping or inside the
    header, a misaligned source, a world below 1."""
    lib = _lib.load()
    bad = lambda rc, name: rc == -1 and name in lib.coocc_last_error()
    chunk = lib.coocc_optim_chunk()
    arena, total = 1 << 20, 2 * chunk + 16                            # header of 2 -> segments at 4 and 12, 5 and 2 chunk + 3 long
    numels = [5, 2 * chunk + 3]

    def tab(seg=(4, 12), src=(256, 260), arena_side="p"):
        t = np.zeros(2, optim.TENSOR_DTYPE)
        t["numel"] = numels
        t[arena_side] = [arena + 4 * s for s in seg]
        t["g" if arena_side == "p" else "p"] = src
        return t

    def pack(t, n=2, nc=4, a=arena, total=total, world=2, dev=one, ch=one):
        return lib.coocc_optim_pack(dev, ctypes.c_void_p(t.ctypes.data) if t is not None else None, n, ch, nc, ctypes.c_void_p(a) if a else None,
                                    total, world, None)

    def unpack(t, n=2, nc=4, a=arena, total=total, dev=one, ch=one):
        return lib.coocc_optim_unpack(dev, ctypes.c_void_p(t.ctypes.data) if t is not None else None, n, ch, nc, ctypes.c_void_p(a) if a else None,
                                      total, None)

    good = tab()
    for f, name, side in ((pack, b"optim_pack", "p"), (unpack, b"optim_unpack", "g")):
        ok = tab(arena_side=side)
        for kw in (dict(dev=None), dict(ch=None)):
            assert bad(f(ok, **kw), name) and b"null table" in lib.coocc_last_error(), (name, kw)
        assert bad(f(None), name) and b"null table" in lib.coocc_last_error()
        for kw in (dict(n=0), dict(nc=0), dict(nc=3), dict(nc=5)):
            assert bad(f(ok, **kw), name), (name, kw)
        assert bad(f(ok, a=0), name) and b"arena" in lib.coocc_last_error()
        assert bad(f(ok, a=arena + 4), name) and b"misaligned arena" in lib.coocc_last_error()
        assert bad(f(tab(seg=(5, 12), arena_side=side)), name) and b"16-byte aligned" in lib.coocc_last_error()
        assert bad(f(tab(seg=(4, 8), arena_side=side)), name) and b"ascending" in lib.coocc_last_error(), "the second overlaps the first"
        assert bad(f(tab(seg=(12, 4), arena_side=side)), name) and b"ascending" in lib.coocc_last_error()
        assert bad(f(ok, total=total - 4), name) and b"outside the arena" in lib.coocc_last_error(), "the last segment ends past the arena"
        assert bad(f(tab(src=(258, 260), arena_side=side)), name) and b"misaligned" in lib.coocc_last_error()
        empty = tab(arena_side=side)
        empty["numel"][0] = 0
        assert bad(f(empty, nc=3), name) and b"numel" in lib.coocc_last_error()
    assert bad(pack(tab(seg=(0, 12))), b"optim_pack") and b"ascending" in lib.coocc_last_error(), "a segment inside the header"
    assert bad(unpack(tab(src=(0, 260), arena_side="g")), b"optim_unpack") and b"destination" in lib.coocc_last_error()
    for world in (0, -2, (1 << 24) + 1):
        assert bad(pack(good, world=world), b"optim_pack") and b"world" in lib.coocc_last_error()
        assert bad(lib.coocc_optim_flag_check(one, 2, one, world, one, None), b"optim_flag_check")
    for args in ((None, 2, one, 2, one), (one, 2, None, 2, one), (one, 2, one, 2, None), (one, 0, one, 2, one)):
        assert bad(lib.coocc_optim_flag_check(*args, None), b"optim_flag_check"), args
