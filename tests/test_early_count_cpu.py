"""Host side of the early result count (host_logic.cpp, early_count_eligible): whether Plan::execute may learn its row count in front of
the root band join's emit pass and return while that pass runs; the option that turns it off; and what has to outlive such an execute — the
retired blocks and the registry of pending tails of tail_lifetime.hpp, driven without a device by tests/host/tail_lifetime_check.cpp."""
import os
import subprocess
import sys

import pytest

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdf-fusion_amd", "csrc")
FLAGS = ("is_root", "result_is_output", "skip_slow", "speculative")      # each must hold
BARS = ("priming", "timing", "option_set")                               # each must not


def test_the_symbols_are_exported():
    lib = rf.load_library()
    for name in ("rdfgpu_early_count_eligible", "rdfgpu_plan_tail_pending"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_the_benchmarks_shape_is_eligible():
    """the steady step of the batched Q5: the band join is the root, emits from the list (counting from the per-row counts at the benchmark's
    size, from the bits on a small store), speculative, untimed"""
    assert rf.early_count_eligible() and rf.early_count_eligible("COUNTS_LIST") and rf.early_count_eligible("VERDICTS_LIST")


@pytest.mark.parametrize("form", ["COUNTS_LIST", "VERDICTS_LIST"])
def test_each_single_condition_flipped_says_no(form):
    for name in FLAGS:
        assert not rf.early_count_eligible(form, **{name: False}), name
    for name in BARS:
        assert not rf.early_count_eligible(form, **{name: True}), name


def test_only_the_list_forms():
    """the other forms' emit passes are not held to what a tail may read (and RECORDS reads the rows' records of a caller-bound table's join)"""
    assert rf.BAND_FORMS == ("RECORDS", "ROW_WINDOWS", "VERDICTS", "VERDICTS_LIST", "COUNTS_LIST")
    for form in ("RECORDS", "ROW_WINDOWS", "VERDICTS"):
        assert not rf.early_count_eligible(form)
    lib = rf.load_library()
    assert lib.rdfgpu_early_count_eligible(1, 1, len(rf.BAND_FORMS), 1, 1, 0, 0, 0) == abi.ERR_INVALID


def test_every_combination_against_the_rule():
    """all 2^7 flag combinations x the five forms: yes exactly where the rule written down in host_logic.hpp says so"""
    names = FLAGS + BARS
    for form in rf.BAND_FORMS:
        for bits in range(1 << len(names)):
            kw = {n: bool(bits >> i & 1) for i, n in enumerate(names)}
            want = form in ("VERDICTS_LIST", "COUNTS_LIST") and all(kw[n] for n in FLAGS) and not any(kw[n] for n in BARS)
            assert rf.early_count_eligible(form, **kw) == want, (form, kw)


def test_the_option_name_round_trips():
    lib = rf.load_library()
    i = abi.OPTIONS["NO_EARLY_RESULT_COUNT"]
    assert abi.OPTION_NAMES[i] == "NO_EARLY_RESULT_COUNT" and lib.rdfgpu_option_name(i) == b"NO_EARLY_RESULT_COUNT"
    assert lib.rdfgpu_option_name(len(abi.OPTION_NAMES)) is None
    # a flag, not a value: it sits among the flags that follow the value options (its environment form is RDFGPU_NO_EARLY_RESULT_COUNT=1)
    assert i > abi.OPTIONS["BAND_PAIR_COUNT_BLOCKS"] and i < abi.OPTIONS["NO_AGG_LDS"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_lifetime_logic_as_a_stand_alone_host_program(sanitize):
    """tests/host/tail_lifetime_check.cpp: execute / execute / complete, two plans interleaved, execute / mutate, destroy with a tail pending, the
    registry under two threads — no block reaches the shared pool while a tail writes it; once more under AddressSanitizer + UBSan."""
    out = subprocess.run(["make", "-C", CSRC, "-s", "tail-lifetime-check"] + (["SANITIZE=1"] if sanitize else []), capture_output=True, text=True)
    sys.stdout.write(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "\n0 failure(s)" in out.stdout
