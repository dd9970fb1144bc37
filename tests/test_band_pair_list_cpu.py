"""Host side of the band join's list of surviving pairs (host_logic.cpp, band_pair_list_eligible; SliceTable::BandRowWindows::pair_list),
and the facts of the small stores that the GPU tests of the list form rely on, from the numpy restatement of the pair test.  No device."""
import numpy as np
import pytest

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
import band_list_cases as bl


def test_option_is_named_and_sits_before_the_pair_cache():
    names = abi.OPTION_NAMES
    i = names.index("NO_BAND_PAIR_LIST")
    assert names[i + 1] == "NO_BAND_PAIR_CACHE" and names[i - 1] == "NO_BAND_ROW_CACHE"
    assert abi.OPTIONS["NO_BAND_PAIR_LIST"] == i
    lib = rf.load_library()
    assert lib.rdfgpu_option_name(i).decode() == "NO_BAND_PAIR_LIST" and lib.rdfgpu_option_name(i + 1).decode() == "NO_BAND_PAIR_CACHE"


@pytest.mark.parametrize("n_blocks", [1, 1392, 203315, (1 << 20) - 1])
def test_the_list_may_cost_what_the_bits_cost(n_blocks):
    """2 bytes per survivor against 512 per block: eligible up to 256 survivors per block on average, not one survivor above"""
    at = 256 * n_blocks
    assert 2 * at == 512 * n_blocks
    assert rf.band_pair_list_eligible(at, n_blocks) and rf.band_pair_list_eligible(0, n_blocks) and rf.band_pair_list_eligible(at - 1, n_blocks)
    assert not rf.band_pair_list_eligible(at + 1, n_blocks)
    assert not rf.band_pair_list_eligible(1 << 40, n_blocks)


def test_not_without_the_cached_verdicts_or_with_the_option():
    assert rf.band_pair_list_eligible(1000, 10, pair_cached=True, option_set=False)
    assert not rf.band_pair_list_eligible(1000, 10, pair_cached=False)
    assert not rf.band_pair_list_eligible(1000, 10, option_set=True)
    assert not rf.band_pair_list_eligible(0, 10, pair_cached=False, option_set=True)


def test_offsets_of_32_bits_cannot_wrap():
    """4096 pairs per block: below 2^20 blocks no total reaches 2^32"""
    assert rf.band_pair_list_eligible(0, (1 << 20) - 1) and not rf.band_pair_list_eligible(0, 1 << 20)
    assert 4096 * ((1 << 20) - 1) < 1 << 32


@pytest.fixture(scope="module")
def small():
    ds = bsbm.generate(2000)
    return ds, bl.feature_pairs(ds)


def test_default_windows_have_blocks_on_both_sides_of_two_round_boundaries(small):
    ds, pairs = small
    per = bl.block_survivors(ds, pairs, 120, 170)
    assert len(per) == 1392
    assert {0, 1, 64, 127, 128, 129, 191, 192, 193} <= set(per.tolist())
    assert round(per.mean()) == 161 and round(2 * per.mean()) == 322
    assert rf.band_pair_list_eligible(int(per.sum()), len(per))
    assert per.max() > 256                                   # (some blocks are longer than the mean the condition allows: it is a mean)


def test_narrow_first_window_has_empty_blocks(small):
    ds, pairs = small
    per = bl.block_survivors(ds, pairs, 7, 900)
    assert int((per == 0).sum()) == 24 and {1, 64} <= set(per.tolist())
    assert rf.band_pair_list_eligible(int(per.sum()), len(per))


def test_wide_windows_decline_the_list(small):
    ds, pairs = small
    per = bl.block_survivors(ds, pairs, 900, 900)
    # 5 127 bytes of list per block against 512 of bits: a mean of 2 563.45 survivors (2 564 when halved from the rounded bytes)
    assert round(2 * per.mean()) == 5127 and abs(per.mean() - 2564) < 1
    assert not rf.band_pair_list_eligible(int(per.sum()), len(per))


def test_list_bytes():
    assert bl.list_bytes(np.array([3, 0, 5])) == 2 * 8 + 4 * 4
