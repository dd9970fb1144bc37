"""The host decision whether a band join that reads a slice's rows in place keeps the pair test's verdicts on the slice
(host_logic.cpp, band_pair_cache_eligible; SliceTable::BandRowWindows::pair_bits).  No device."""
import rdf_fusion_amd as rf
from rdf_fusion_amd import abi

Q5_BLOCKS = 203385          # blocks of the productFeature slice's in-place layout at 285 000 products
AUTO = 1 << 21              # BAND_PAIR_CACHE_BLOCKS = 0


def test_q5_shape_is_eligible():
    assert rf.band_pair_cache_eligible(Q5_BLOCKS)
    assert rf.band_pair_cache_eligible(0) and rf.band_pair_cache_eligible(1)


def test_each_condition_declines_on_its_own():
    assert not rf.band_pair_cache_eligible(Q5_BLOCKS, row_windows=False)      # the rows' windows are not kept (not eligible, or declined for this store)
    assert not rf.band_pair_cache_eligible(Q5_BLOCKS, neq_self=False)         # the `!=` compares ids, not entry indices
    assert not rf.band_pair_cache_eligible(Q5_BLOCKS, pack16=False)           # 32-bit windows
    assert not rf.band_pair_cache_eligible(Q5_BLOCKS, option_set=True)        # NO_BAND_PAIR_CACHE
    assert not rf.band_pair_cache_eligible(Q5_BLOCKS, cap_blocks=Q5_BLOCKS - 1)
    assert rf.band_pair_cache_eligible(Q5_BLOCKS, row_windows=True, neq_self=True, pack16=True, option_set=False, cap_blocks=Q5_BLOCKS)


def test_the_cap_is_inclusive():
    for cap in (1, 64, Q5_BLOCKS, (1 << 31) - 1):
        assert rf.band_pair_cache_eligible(cap, cap_blocks=cap)
        assert rf.band_pair_cache_eligible(cap - 1, cap_blocks=cap)
        assert not rf.band_pair_cache_eligible(cap + 1, cap_blocks=cap)


def test_zero_means_two_to_the_21():
    assert rf.band_pair_cache_eligible(AUTO) and rf.band_pair_cache_eligible(AUTO, cap_blocks=0)
    assert not rf.band_pair_cache_eligible(AUTO + 1)
    assert rf.band_pair_cache_eligible(AUTO + 1, cap_blocks=AUTO + 1)          # an explicit cap may lie above the automatic one
    assert not rf.band_pair_cache_eligible(1 << 40)


def test_the_options_are_named_and_sit_before_the_last():
    names = abi.OPTION_NAMES
    i = names.index("NO_BAND_PAIR_CACHE")
    assert names[i + 1] == "BAND_PAIR_CACHE_BLOCKS" and names[i + 2] == "NO_AGG_LDS" and i + 3 == len(names)
    lib = rf.load_library()
    assert lib.rdfgpu_option_name(i).decode() == "NO_BAND_PAIR_CACHE" and lib.rdfgpu_option_name(i + 1).decode() == "BAND_PAIR_CACHE_BLOCKS"
