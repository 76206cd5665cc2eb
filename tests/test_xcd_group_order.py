"""The block-order functions of csrc/common.h on the host (tstar_xcd_group_block runs the very function the kernels call).

xcd_remap_groups(bid, ngroups, gsize): hardware block bid sits on XCD bid % 8; the gsize blocks of a group (the query tiles of one
(image, head) in attention_x3_kernel) must all sit on ONE XCD, consecutively in that XCD's order, every logical block must be
computed exactly once, and the padding blocks (-1) are fewer than 8 groups' worth."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from tstar_amd import _lib
    return _lib.load()


def _table(lib, ngroups, gsize):
    grid = lib.tstar_xcd_groups_grid(ngroups, gsize)
    return grid, [lib.tstar_xcd_group_block(b, ngroups, gsize) for b in range(grid)]


@pytest.mark.parametrize("gsize", [1, 2, 3, 5, 6])
def test_bijection_and_one_xcd_per_group(lib, gsize):
    """Every block count ngroups * gsize up to 200 and a few groups beyond (for gsize = 1: every count 1..209)."""
    for ngroups in range(1, 200 // gsize + 10):
        grid, m = _table(lib, ngroups, gsize)
        assert grid % 8 == 0 and 0 <= grid - ngroups * gsize < 8 * gsize
        live = [(b, x) for b, x in enumerate(m) if x != -1]
        assert sorted(x for _, x in live) == list(range(ngroups * gsize)), (ngroups, gsize)      # onto, each once
        per_xcd = {}
        for b, x in live:
            per_xcd.setdefault(b % 8, []).append(x)
        groups_seen = set()
        for xcd, xs in per_xcd.items():
            # an XCD runs its blocks in bid order: whole groups, members in order, one group after the other
            assert len(xs) % gsize == 0
            for i in range(0, len(xs), gsize):
                g = xs[i] // gsize
                assert xs[i:i + gsize] == list(range(g * gsize, (g + 1) * gsize)), (ngroups, gsize, xcd)
                assert g not in groups_seen
                groups_seen.add(g)
        assert len(groups_seen) == ngroups
        loads = [len(per_xcd.get(x, [])) // gsize for x in range(8)]
        assert max(loads) - min(loads) <= 1                                                      # groups spread evenly over the XCDs


def test_bench_shapes(lib):
    """T = 577 -> five query tiles; 12 heads: B = 1 is 60 blocks (not a multiple of 8), B = 3 is 180."""
    for B in (1, 3, 350):
        grid, m = _table(lib, B * 12, 5)
        for g in range(B * 12):
            assert len({b % 8 for b, x in enumerate(m) if x != -1 and x // 5 == g}) == 1


def test_arguments(lib):
    assert lib.tstar_xcd_groups_grid(0, 5) == -1 and lib.tstar_xcd_groups_grid(3, 0) == -1
    assert lib.tstar_xcd_group_block(-1, 3, 5) == -2 and lib.tstar_xcd_group_block(40, 3, 5) == -2
    assert lib.tstar_xcd_groups_grid(3, 5) == 40
