"""Host side of the ordered slice join's probe pass (host_logic.cpp, oj_probe_form): whether that join owes its probe to the band join above it, and
which pass settles the debt, over every combination of the decision's inputs.  No device."""
import itertools

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi


def test_the_symbol_is_exported_and_the_names_are_the_enum():
    assert "rdfgpu_oj_probe_form" in abi.EXPORTED_SYMBOLS
    assert hasattr(rf.load_library(), "rdfgpu_oj_probe_form")
    assert rf.OJ_PROBE_FORMS == ("FULL", "LEAN", "FULL_NOW")


def test_every_combination_of_the_inputs():
    seen = set()
    for held, in_place, row_cache, option_set, row_static in itertools.product([False, True], repeat=5):
        got = rf.oj_probe_form(held=held, in_place=in_place, row_cache=row_cache, option_set=option_set, row_static=row_static)
        owed = held and in_place and row_cache and not option_set          # what run_ordered_join asks: the same flags with row_static = True
        asked_by_the_join = rf.oj_probe_form(held=held, in_place=in_place, row_cache=row_cache, option_set=option_set, row_static=True)
        assert (asked_by_the_join != "FULL") == owed, (held, in_place, row_cache, option_set)
        if got == "LEAN":                                                  # only for held, in place, row cache, option off
            assert held and in_place and row_cache and not option_set and row_static
        if owed and not row_static:                                        # a lean probe is owed and the step is not row_static
            assert got == "FULL_NOW"
        expected = "FULL" if not owed else "LEAN" if row_static else "FULL_NOW"
        assert got == expected, (held, in_place, row_cache, option_set, row_static, got)
        seen.add(got)
    assert seen == set(rf.OJ_PROBE_FORMS)


def test_the_defaults_are_the_steady_step():
    assert rf.oj_probe_form() == "LEAN"
    assert rf.oj_probe_form(row_static=False) == "FULL_NOW"
    for off in ("held", "in_place", "row_cache"):
        assert rf.oj_probe_form(**{off: False}) == "FULL" and rf.oj_probe_form(row_static=False, **{off: False}) == "FULL"
    assert rf.oj_probe_form(option_set=True) == "FULL" and rf.oj_probe_form(option_set=True, row_static=False) == "FULL"
