"""Host side of the band join's per-row counts (host_logic.cpp, band_pair_count_eligible; SliceTable::BandRowWindows::pair_cnt), and the facts of
the small stores that the GPU tests of the counts form rely on, from the numpy restatement of the pair test.  No device."""
import numpy as np
import pytest

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
import band_list_cases as bl
import band_count_cases as bc

AUTO = 1 << 16              # BAND_PAIR_COUNT_BLOCKS = 0: 32 MiB of verdicts
Q5_BLOCKS = 203385          # blocks of the productFeature slice's in-place layout at 285 000 products


def test_options_are_named_and_leave_the_pinned_neighbours_alone():
    names = abi.OPTION_NAMES
    i = names.index("NO_BAND_PAIR_COUNTS")
    assert names[i + 1] == "BAND_PAIR_COUNT_BLOCKS" and names.index("BAND_PAIR_COUNT_BLOCKS") < names.index("NO_AGG_LDS")
    assert names[-1] == "NO_AGG_LDS"
    assert abi.OPTIONS["NO_BAND_PAIR_COUNTS"] == i and abi.OPTIONS["BAND_PAIR_COUNT_BLOCKS"] == i + 1
    lib = rf.load_library()
    assert lib.rdfgpu_option_name(i).decode() == "NO_BAND_PAIR_COUNTS" and lib.rdfgpu_option_name(i + 1).decode() == "BAND_PAIR_COUNT_BLOCKS"
    assert "rdfgpu_band_pair_count_eligible" in abi.EXPORTED_SYMBOLS


@pytest.mark.parametrize("n", [1, 2, 1383, 1392, AUTO + 1, Q5_BLOCKS, 1 << 20])
def test_the_bound_is_inclusive(n):
    assert rf.band_pair_count_eligible(n, min_blocks=n)
    assert not rf.band_pair_count_eligible(n - 1, min_blocks=n)
    assert rf.band_pair_count_eligible(n + 1, min_blocks=n)


def test_zero_means_two_to_the_16():
    assert 512 * AUTO == 32 << 20
    assert rf.band_pair_count_eligible(AUTO) and rf.band_pair_count_eligible(AUTO, min_blocks=0)
    assert not rf.band_pair_count_eligible(AUTO - 1) and not rf.band_pair_count_eligible(AUTO - 1, min_blocks=0)
    assert rf.band_pair_count_eligible(AUTO - 1, min_blocks=AUTO - 1)          # an explicit bound may lie below the automatic one
    assert rf.band_pair_count_eligible(Q5_BLOCKS) and not rf.band_pair_count_eligible(1392) and not rf.band_pair_count_eligible(0)


def test_not_without_the_list_or_with_the_option():
    assert rf.band_pair_count_eligible(Q5_BLOCKS, has_list=True, option_set=False)
    assert not rf.band_pair_count_eligible(Q5_BLOCKS, has_list=False)
    assert not rf.band_pair_count_eligible(Q5_BLOCKS, option_set=True)
    assert not rf.band_pair_count_eligible(Q5_BLOCKS, has_list=False, option_set=True)
    assert not rf.band_pair_count_eligible(10, has_list=False, min_blocks=1) and not rf.band_pair_count_eligible(10, option_set=True, min_blocks=1)


@pytest.fixture(scope="module")
def small():
    ds = bsbm.generate(2000)
    return ds, bl.feature_pairs(ds)


def test_row_counts_add_up_to_the_blocks_survivors(small):
    ds, pairs = small
    for w1, w2 in ((120, 170), (7, 900)):
        rc = bc.row_counts(ds, pairs, w1, w2)
        np.testing.assert_array_equal(rc.sum(axis=1), bl.block_survivors(ds, pairs, w1, w2))


def test_default_windows_count_at_most_16_per_row(small):
    ds, pairs = small
    rc = bc.row_counts(ds, pairs, 120, 170)
    assert rc.shape == (1392, 64) and rc.max() == 16
    assert rf.band_pair_list_eligible(int(rc.sum()), len(rc))
    assert rf.band_pair_count_eligible(len(rc), min_blocks=1) and not rf.band_pair_count_eligible(len(rc))


def test_one_literal_for_the_largest_group_fills_rows(small):
    """the largest feature group, 139 products = chunks of 64, 64 and 11 rows: with one numeric1 and one numeric2 for all of them its two
    off-diagonal blocks of 64 x 64 are full and the last row chunk's 11 rows count 64 in two blocks more: 2 * 64 + 2 * 11 = 150 counts of 64"""
    ds, pairs = small
    f, products = bc.largest_group(ds, pairs)
    assert len(products) == 139
    old, new, v1, v2 = bc.full_rows_edit(ds, pairs)
    assert len(old[0]) == len(new[0]) == 2 * 139
    rc = bc.row_counts(ds, pairs, 120, 170, v1, v2)
    per = bl.block_survivors(ds, pairs, 120, 170, v1, v2)
    assert rc.max() == 64 and int((rc == 64).sum()) == 150 == 2 * 64 + 2 * 11
    assert int((per == 4096).sum()) == 2 and per.max() == 4096
    assert per.mean() < 256 and rf.band_pair_list_eligible(int(per.sum()), len(per))   # (a mean of 178 survivors per block)
    assert round(per.mean()) == 178


def test_edge_store_ends_mid_group_for_every_wave_width():
    """the store of test_group_and_block_edges: 1 383 blocks, odd, 3 mod 4 and 7 mod 16 — a wave taking 2, 4, 8 or 16 blocks ends mid-group"""
    ds = bsbm.generate(2000)
    pairs = bl.feature_pairs(ds)
    kept = bc.edge_store_pairs(ds, pairs)[0]
    chunks = (np.unique(kept[:, 1], return_counts=True)[1] + 63) // 64
    n_blocks = int((chunks * chunks).sum())
    assert n_blocks == 1383 and n_blocks % 2 == 1 and n_blocks % 4 == 3 and n_blocks % 8 == 7 and n_blocks % 16 == 7
