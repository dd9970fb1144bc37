"""The integer-window cases of band_cases.py on the CPU: the oracle's operator-at-a-time answer must be the Python-int reference's on every
case the device tests run (test_gpu_band_edges.py), so that a wrong reference cannot hide a device bug, and the inputs must be worth
running: most cases neither empty nor the whole unfiltered join, the cases meant to be empty empty."""
import numpy as np
import pytest

from oracle import oracle as orc
import band_cases as bc
import kat_util as ku

I64_MIN, I64_MAX = bc.I64_MIN, bc.I64_MAX


def oracle_store(st):
    os_ = orc.OracleStore()
    os_.extend(*st.quads)
    os_.set_typed_values(st.tv, st.decimals)
    return os_


def test_value_sets_sit_on_both_sides_of_every_limit():
    spreads = {vs.spread for vs in bc.VALUE_SETS}
    for limit in (bc.PACK_SPREAD_MAX + 1, bc.BAND_SPREAD_LIMIT, bc.INDEX_SPREAD_LIMIT):
        assert limit in spreads and limit - 1 in spreads, hex(limit)
    assert any(vs.has_min and I64_MIN in vs.values for vs in bc.VALUE_SETS)
    assert any(max(vs.values) - min(vs.values) == 2 ** 64 - 2 for vs in bc.VALUE_SETS)
    for vs in bc.VALUE_SETS:
        assert all(I64_MIN <= v <= I64_MAX for v in vs.values + vs.y_values), vs.name
        assert max(vs.values) - min(vs.values) == vs.spread, vs.name
    assert {min(vs.values) for vs in bc.VALUE_SETS} >= {I64_MIN + 1, -2 ** 62, -3}
    assert sum(max(vs.values) == I64_MAX for vs in bc.VALUE_SETS) >= len(bc.SPREADS)


def test_store_geometry():
    st = bc.store_of(bc.VALUE_SETS[1])
    g, s, p, o = st.quads
    q = np.unique(np.stack([s[p == bc.PF], o[p == bc.PF]], axis=1), axis=0)
    sizes = np.bincount(q[:, 1] - bc.FEAT0, minlength=bc.N_FEAT)
    assert {0, 1, 63, 64, 65, 128, 129, 512} <= set(sizes.tolist()) and sizes.max() == 512
    assert len(q) == st.n_build > 1024 and len(q) >= 4 * bc.N_FEAT and len(q) < len(s[p == bc.PF])      # (duplicates went in)
    per_key = np.bincount(st.T[2], minlength=bc.FEAT0 + bc.N_FEAT + 1)
    assert {0, 1, 63, 64, 65, 129} <= set(per_key[bc.FEAT0:bc.FEAT0 + bc.N_FEAT].tolist())
    assert per_key[0] == 20 and (st.T[1] == 0).any() and (st.T[3] == 0).any() and 1300 < len(st.T[0]) < 1600
    assert all((p == pv).sum() > 1024 for pv in (bc.PV, bc.PV2))
    big = bc.store_of(bc.VALUE_SETS[1], big_group=True)
    g, s, p, o = big.quads
    assert np.bincount(o[p == bc.PF]).max() == 513


def test_reference_model_known_answers():
    w = bc.Window("w", "LT", False, 1, "GT", True, 1)
    i = lambda v: ("integer", v)
    assert bc.window_holds(w, i(5), i(5), None) and not bc.window_holds(w, i(6), i(5), None) and not bc.window_holds(w, i(4), i(5), None)
    assert not bc.window_holds(w, i(I64_MAX), i(I64_MAX), None)            # y + 1 is no xsd:integer of this store: an error
    assert not bc.window_holds(w, i(I64_MIN), i(I64_MIN), None)
    assert bc.window_holds(w, i(I64_MIN + 1), i(I64_MIN + 1), None)
    assert not bc.window_holds(w, i(5), None, None)
    assert bc.window_holds(w, i(5), ("double", 5.5), None) and not bc.window_holds(w, i(5), ("double", float("nan")), None)
    assert bc.window_holds(w, i(12), ("decimal", bc.Fraction(25, 2)), None) and not bc.window_holds(w, i(14), ("decimal", bc.Fraction(25, 2)), None)
    # doubles round: 2^62 + 1 and 2^62 are one double, so `<` fails where the integers would pass
    w2 = bc.Window("w2", "LT", False, 0, "GEQ", True, 0)
    assert not bc.window_holds(w2, i(2 ** 62), ("double", float(2 ** 62)), None)
    w3 = bc.Window("w3", "LT", True, I64_MIN, "GEQ", False, 0)
    assert bc.window_holds(w3, i(-1), i(-1), None) and not bc.window_holds(w3, i(0), i(0), None)


_REFS = {}


def references(k):
    """(store, [(case, expected rows, unfiltered rows)]) of value set k: computed once, shared by the tests below and left unchanged"""
    if k not in _REFS:
        st = bc.store_of(bc.VALUE_SETS[k])
        _REFS[k] = (st, [(c,) + bc.window_reference(st.quads, st.terms, st.T, c.windows, c.neq) for c in bc.cases_of(k)])
    return _REFS[k]


@pytest.mark.parametrize("k", range(len(bc.VALUE_SETS)), ids=[vs.name for vs in bc.VALUE_SETS])
def test_oracle_equals_reference(k):
    vs = bc.VALUE_SETS[k]
    st, refs = references(k)
    os_ = oracle_store(st)
    for c, want, unfiltered in refs:
        exp, n_exp, _ = os_.execute(bc.band_plan(c.windows, c.neq), [st.T])
        assert n_exp == len(want), (vs.name, bc.case_id(c), n_exp, len(want))
        np.testing.assert_array_equal(ku.multiset(exp, n_exp), want, err_msg=f"{vs.name} {bc.case_id(c)}")
    want, _ = bc.window_reference(st.quads, st.terms, st.T_int, (bc.ZERO_WINDOW,), True)
    exp, n_exp, _ = os_.execute(bc.band_plan((bc.ZERO_WINDOW,), True), [st.T_int])
    np.testing.assert_array_equal(ku.multiset(exp, n_exp), want, err_msg=f"{vs.name} all-integer table")
    assert 0 < len(want), vs.name


def test_oracle_equals_reference_with_a_group_of_513():
    vs = bc.VALUE_SETS[1]
    st = bc.store_of(vs, big_group=True)
    os_ = oracle_store(st)
    for c in bc.cases_of(1)[:2]:
        want, unfiltered = bc.window_reference(st.quads, st.terms, st.T, c.windows, c.neq)
        exp, n_exp, _ = os_.execute(bc.band_plan(c.windows, c.neq), [st.T])
        np.testing.assert_array_equal(ku.multiset(exp, n_exp), want, err_msg=bc.case_id(c))
        assert 0 < len(want) < unfiltered


def test_cases_are_not_trivial():
    """At least three quarters of the cases have a result that is neither empty nor the unfiltered join; every case with a window meant
    to be empty is empty; every window and every value set decides some non-trivial case."""
    results = {}
    for k, vs in enumerate(bc.VALUE_SETS):
        for c, want, unfiltered in references(k)[1]:
            results[(vs.name, bc.case_id(c))] = (len(want), unfiltered, any(w.empty for w in c.windows))
    good = {key for key, (n, unfiltered, empty) in results.items() if 0 < n < unfiltered}
    for key, (n, unfiltered, empty) in results.items():
        assert not empty or n == 0, key
        assert unfiltered > 1000, key
    print(f"{len(good)} of {len(results)} cases are non-trivial")
    assert 4 * len(good) >= 3 * len(results), sorted(set(results) - good)
    for w in bc.WINDOWS:
        assert w.empty or any(w.name in cid for _, cid in good), w.name
    for vs in bc.VALUE_SETS:
        assert any(name == vs.name for name, _ in good), vs.name
    # every window decides a non-trivial case in each regime: packed records, 32-bit records, no band join
    regime = {vs.name: "refused" if vs.has_min or vs.spread >= bc.BAND_SPREAD_LIMIT else "packed" if vs.spread <= bc.PACK_SPREAD_MAX else "wide" for vs in bc.VALUE_SETS}
    for w in bc.WINDOWS:
        met = {regime[vs.name] for k, vs in enumerate(bc.VALUE_SETS) for c, want, unfiltered in references(k)[1] if w in c.windows and 0 < len(want) < unfiltered}
        assert w.empty or met == {"packed", "wide", "refused"}, (w.name, met)
