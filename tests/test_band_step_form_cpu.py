"""Host side of the band join's forms (host_logic.cpp, band_step_form; the table of the forms heads band_join.hip): the one decision of how a step runs,
against a Python statement of the rules it replaced — the host's route flags, the kernel-argument pointers set from them, and what the two launchers
made of those pointers — over the full truth table.  No device."""
import itertools

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi

AUTO = 1 << 16              # BAND_PAIR_COUNT_BLOCKS = 0
BLOCKS = [0, 1391, 1392, 1393, AUTO - 1, AUTO]
MIN_BLOCKS = [0, 1, 1392, 1393]
FORM_OF_PASSES = {("records", "records"): "RECORDS", ("static", "static"): "ROW_WINDOWS", ("cached", "cached"): "VERDICTS",
                  ("cached", "list"): "VERDICTS_LIST", ("counts", "list"): "COUNTS_LIST"}


def passes_before(row_static, has_verdicts, has_list, list_option_set, counts_option_set, n_row_cols, blocks, min_blocks):
    """(mask pass, emit pass) as they were chosen before the form had a name."""
    # the route flags and what the step took of the slice's tables (a plan whose options decline the list does not use one another plan left)
    pair_cached = row_static and has_verdicts
    pair_list = has_verdicts and has_list and not list_option_set
    counts = pair_cached and pair_list and n_row_cols <= 1 and not counts_option_set and blocks >= (min_blocks if min_blocks else AUTO)
    # the kernel arguments
    row_win = row_static
    bvalid = pair_cached and not counts
    pair_cnt = counts
    list_ptr = (counts or pair_cached) and pair_list
    # the launchers' reading of them
    mask = "counts" if row_win and pair_cnt else "cached" if row_win and bvalid else "static" if row_win else "records"
    emit = ("list" if row_win and (bvalid or pair_cnt) and list_ptr and n_row_cols <= 1 else
            "cached" if row_win and bvalid else "static" if row_win else "records")
    return mask, emit


def test_the_symbol_is_exported_and_the_names_are_the_enum():
    assert "rdfgpu_band_step_form" in abi.EXPORTED_SYMBOLS
    assert hasattr(rf.load_library(), "rdfgpu_band_step_form")
    assert rf.BAND_FORMS == ("RECORDS", "ROW_WINDOWS", "VERDICTS", "VERDICTS_LIST", "COUNTS_LIST")
    assert set(FORM_OF_PASSES.values()) == set(rf.BAND_FORMS)


def test_the_form_is_what_flags_pointers_and_launchers_chose_before():
    seen = set()
    for flags in itertools.product([False, True], repeat=5):
        for n_row_cols, blocks, min_blocks in itertools.product([0, 1, 2], BLOCKS, MIN_BLOCKS):
            row_static, has_verdicts, has_list, list_option_set, counts_option_set = flags
            before = passes_before(*flags, n_row_cols, blocks, min_blocks)
            assert before in FORM_OF_PASSES, (flags, n_row_cols, blocks, min_blocks, before)      # the two launchers agreed on every input
            got = rf.band_step_form(blocks, row_static=row_static, has_verdicts=has_verdicts, has_list=has_list, list_option_set=list_option_set,
                                    counts_option_set=counts_option_set, n_row_cols=n_row_cols, min_blocks=min_blocks)
            assert got == FORM_OF_PASSES[before], (flags, n_row_cols, blocks, min_blocks, got, before)
            seen.add(got)
    assert seen == set(rf.BAND_FORMS)


def test_the_facts_the_gpu_tests_rely_on():
    assert rf.band_step_form(1392) == "VERDICTS_LIST" and rf.band_step_form(1383) == "VERDICTS_LIST"      # the 2 000-product stores, default options
    assert rf.band_step_form(1392, min_blocks=1) == "COUNTS_LIST" and rf.band_step_form(1383, min_blocks=1) == "COUNTS_LIST"
    assert rf.band_step_form(1392, min_blocks=1, counts_option_set=True) == "VERDICTS_LIST"
    assert rf.band_step_form(1392, min_blocks=1392) == "COUNTS_LIST" and rf.band_step_form(1392, min_blocks=1393) == "VERDICTS_LIST"   # inclusive
    assert rf.band_step_form(AUTO) == "COUNTS_LIST" and rf.band_step_form(AUTO - 1) == "VERDICTS_LIST"
    assert rf.band_step_form(1392, list_option_set=True) == "VERDICTS" and rf.band_step_form(1392, has_list=False) == "VERDICTS"
    assert rf.band_step_form(1392, n_row_cols=2, min_blocks=1) == "VERDICTS"                              # the list form knows one row column
    assert rf.band_step_form(1392, has_verdicts=False) == "ROW_WINDOWS" and rf.band_step_form(AUTO, has_verdicts=False, min_blocks=1) == "ROW_WINDOWS"
    for has_verdicts, has_list, blocks, min_blocks in itertools.product([False, True], [False, True], BLOCKS, MIN_BLOCKS):
        assert rf.band_step_form(blocks, row_static=False, has_verdicts=has_verdicts, has_list=has_list, min_blocks=min_blocks) == "RECORDS"
