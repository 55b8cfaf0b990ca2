"""CPU: the size of the routed scatter's counter block and scratch (csrc/hashgrid.hip make_plan) as the library reports them,
against the layout the tests read the block with (_lib.hashgrid_counter_layout).  The block is {bin counts | queue head +
tickets (4) | arrivals | first item | parts}: the parts do not overlap, everything a call must leave at zero comes first, and
against the block without arrival counters (3 words per bin) the scratch grows by what the longer block pushes the records
back -- nothing else.  (That the kernels use these offsets is held on the GPU: tests/test_gpu_scatter_fold.py finds the
plan's parts of every bin at `parts` and zeros in front of `first`.)"""
import math

import pytest

from mipsfusion_amd import _lib

PLS = float(2.0 ** (math.log2(256 / 16) / 15))
SC_MAX_SLICE, SC_SLICE_LOG2, SC_PART, SC_PART_DENSE = 8192, 13, 24576, 8192


def n_bins(meta):
    total = 0
    for l in range(meta.n_levels):
        size = meta.offsets[l + 1] - meta.offsets[l]
        total += 1 if size <= SC_MAX_SLICE else (size + (1 << SC_SLICE_LOG2) - 1) >> SC_SLICE_LOG2
    return total


def up(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("table", [10, 13, 14, 19, 22])
def test_counter_block_layout(table):
    meta = _lib.make_grid_meta(16, 2, table, 16, PLS)
    w = _lib.hashgrid_counter_layout(meta)
    bins = n_bins(meta)
    assert w["n_bins"] == bins
    spans = [(w["count"], bins), (w["nitems"], 4), (w["arrive"], bins), (w["first"], bins), (w["parts"], bins)]
    assert spans[0][0] == 0
    for (a, n), (b, _) in zip(spans, spans[1:]):
        assert a + n == b, "the parts of the block follow each other without a gap or an overlap"
    assert w["end"] == up(w["parts"] + bins, 4) == up(4 * bins + 4, 4)
    assert w["end"] == _lib.buffer_size(_lib.SIZE_HASHGRID_COUNTER_WORDS, meta=meta)
    # what every call leaves at zero is the front of the block: counts, head, tickets, arrivals
    assert w["first"] == 2 * bins + 4


@pytest.mark.parametrize("M", [1, 64, 8193, 262144])
@pytest.mark.parametrize("table", [14, 19])
def test_scratch_grows_by_the_arrival_counters_only(table, M):
    meta = _lib.make_grid_meta(16, 2, table, 16, PLS)
    bins = n_bins(meta)
    w = _lib.hashgrid_counter_layout(meta)

    def scratch(block_words):
        rec = up(block_words, 16)
        part = up(rec + bins * M, 16)
        max_items = (8 * 16 * M + min(SC_PART, SC_PART_DENSE) - 1) // min(SC_PART, SC_PART_DENSE) + bins
        return part + max_items * SC_MAX_SLICE * 2 + 64

    got = _lib.buffer_size(_lib.SIZE_HASHGRID_BWD_SCRATCH, M, 0, 0, meta)
    assert got == scratch(w["end"])
    before = scratch(up(3 * bins + 4, 4))
    assert 0 <= got - before <= up(bins, 16) + 16, "only the arrival counters were added"
    assert _lib.buffer_size(_lib.SIZE_HASHGRID_BWD_SCRATCH, M, 1, 0, meta) == got + 16 * M * 3
