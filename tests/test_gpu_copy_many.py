"""``coocc_copy_many`` (csrc/layout.hip): up to 16 device -> device copies as one launch, against the sources byte for byte.
Item sizes from 0 bytes to 1 MiB + 4, sources and destinations 0, 4 and 8 bytes past a 16-byte boundary (the 16-byte vector path,
the 4-byte word path and their tails), 1, 2 and 16 items per launch; the guard bytes on both sides of every destination stay as
they were; a bad item count is refused before anything is launched."""
import pytest
import torch

from co_occ_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 4, 12, 36, 60, 156, (1 << 20) + 4)
OFFSETS = (0, 4, 8)
GUARD = 64            # bytes on each side of a destination
FILL = 0xA5


def _span(nbytes):
    return (nbytes + 15) // 16 * 16 + 32          # room for the item at any of OFFSETS, on a 16-byte grid


class _Arena:
    """Sources (random bytes) and guarded destinations (FILL everywhere) of a list of (bytes, src offset, dst offset) items, each
    carved from one buffer on a 16-byte grid."""

    def __init__(self, items, dev, seed):
        g = torch.Generator().manual_seed(seed)
        self.items = items
        total_s = sum(_span(b) for b, _, _ in items) + 16
        total_d = sum(_span(b) + 2 * GUARD for b, _, _ in items) + 16
        self.src = torch.randint(0, 256, (total_s,), dtype=torch.uint8, generator=g).to(dev)
        self.dst = torch.full((total_d,), FILL, dtype=torch.uint8, device=dev)
        base_s = -self.src.data_ptr() % 16
        base_d = -self.dst.data_ptr() % 16
        self.at = []                                  # (src start, dst start, bytes): element offsets into src / dst
        ps, pd = base_s, base_d
        for b, so, do in items:
            self.at.append((ps + so, pd + GUARD + do, b))
            ps += _span(b)
            pd += _span(b) + 2 * GUARD
        self.table = (_lib.CopyItem * max(1, len(items)))()
        for it, (s0, d0, b) in zip(self.table, self.at):
            it.dst, it.src, it.bytes = self.dst.data_ptr() + d0, self.src.data_ptr() + s0, b

    def expected(self):
        want = torch.full_like(self.dst, FILL)
        for s0, d0, b in self.at:
            want[d0:d0 + b] = self.src[s0:s0 + b]
        return want


def _launch(arena, n=None):
    lib = _lib.load()
    rc = lib.coocc_copy_many(arena.table, len(arena.items) if n is None else n, _lib.stream(arena.dst.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("src_off", OFFSETS)
@pytest.mark.parametrize("dst_off", OFFSETS)
def test_one_item_of_every_size_at_every_alignment(dev, src_off, dst_off):
    for size in SIZES:
        a = _Arena([(size, src_off, dst_off)], dev, seed=size % 97 + src_off + 3 * dst_off)
        assert a.table[0].src % 16 == src_off and a.table[0].dst % 16 == dst_off
        assert _launch(a) == 0
        assert torch.equal(a.dst, a.expected()), "size %d, src +%d, dst +%d" % (size, src_off, dst_off)


def test_two_items_a_large_one_beside_a_matrix(dev):
    for big_first in (True, False):
        items = [((1 << 20) + 4, 0, 0), (36, 4, 8)]
        a = _Arena(items if big_first else items[::-1], dev, seed=11)
        assert _launch(a) == 0
        assert torch.equal(a.dst, a.expected())


def test_sixteen_items_of_mixed_sizes_and_alignments(dev):
    items = [(SIZES[i % len(SIZES)], OFFSETS[i % 3], OFFSETS[(i // 3) % 3]) for i in range(16)]
    assert {b for b, _, _ in items} == set(SIZES)
    a = _Arena(items, dev, seed=16)
    assert _launch(a) == 0
    want = a.expected()
    assert torch.equal(a.dst, want)
    # the same table once more with other contents: only the sources' bytes changed, the table is reused as the serving loop does
    a.src.copy_(torch.randint(0, 256, a.src.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(17)).to(dev))
    assert _launch(a) == 0
    assert torch.equal(a.dst, a.expected()) and not torch.equal(a.dst, want)


def test_a_bad_item_count_is_refused_before_anything_is_launched(dev):
    lib = _lib.load()
    a = _Arena([(156, 0, 0)] * 17, dev, seed=3)
    for n in (0, 17, -1):
        assert _launch(a, n) == -1 and b"copy_many" in lib.coocc_last_error()
        assert bool((a.dst == FILL).all()), "n = %d wrote something" % n
    assert lib.coocc_copy_many(None, 1, None) == -1
    a.table[1].src = None                        # a null source in a non-empty item
    assert _launch(a, 2) == -1 and bool((a.dst == FILL).all())
    a.table[1].bytes = 0                         # ... is fine once the item is empty
    assert _launch(a, 2) == 0
    assert torch.equal(a.dst[a.at[0][1]:a.at[0][1] + 156], a.src[a.at[0][0]:a.at[0][0] + 156])
