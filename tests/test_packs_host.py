"""Host logic of the weight packs (lighthand_amd/weight_packs.py): the early / late split of the tiled pack launch and the work-item tables
of the two pack kernels, as pure functions of the layer sizes.  No GPU, no kernel library."""
import numpy as np
import pytest

from lighthand_amd.weight_packs import late_pack_split, pack_chunk_table, pack_tile_table


@pytest.mark.parametrize("sizes,want", [
    ([7] * 15, None),                       # fewer than 16 convolutions
    ([1] * 20, None),                       # the tail of <= 0.8 of the total starts at conv 4: fewer than 8 layers in front of it
    ([1] * 12 + [10] * 8, (13, 5)),         # total 92: seven 10s (70 <= 73.6) are late; fork 13 - max(8, int(0.35 * 20)) = 5
    ([1] * 8 + [100] * 8, (10, 2)),         # total 808: six 100s (600 <= 646.4) are late; fork 10 - max(8, int(0.35 * 16)) = 2
    ([1] * 19 + [100], None),               # the last layer alone exceeds 0.8 of the total: nothing can be late
])
def test_late_pack_split_follows_the_rule(sizes, want):
    assert late_pack_split(sizes) == want


def test_tile_table_is_row_major_per_conv():
    dims = [(33, 64), (32, 31)]
    want = [(0, a, b) for a in range(2) for b in range(2)] + [(1, 0, 0)]         # ceil(33/32) * ceil(64/32) = 4 tiles, then 1 * 1
    assert pack_tile_table(dims) == want
    for i, (d0, d1) in enumerate(dims):
        assert sum(1 for t in want if t[0] == i) == -(-d0 // 32) * -(-d1 // 32)


@pytest.mark.parametrize("chunk", [1, 1000, 4096, 1 << 20])
@pytest.mark.parametrize("kstep", [32, 64])
def test_chunk_table_covers_every_padded_element_once(chunk, kstep):
    items = [(70, 33, 9), (128, 64, 1), (1, 1, 1), (129, 65, 4)]               # (n_out, n_in, ntaps)
    if chunk == 1:
        items = items[2:3]                                                     # one chunk per element: the smallest image is enough
    table = pack_chunk_table(items, chunk, kstep)
    assert [i for i, _ in table] == sorted(i for i, _ in table)                # grouped by item, in order
    for i, (n_out, n_in, ntaps) in enumerate(items):
        total = -(-n_out // 128) * 128 * ntaps * -(-n_in // kstep) * kstep
        hits = np.zeros(total, dtype=np.int32)
        for _, s0 in (t for t in table if t[0] == i):
            assert 0 <= s0 < total
            hits[s0:s0 + chunk] += 1                                           # a work item packs [start, min(start + chunk, total))
        assert (hits == 1).all()
