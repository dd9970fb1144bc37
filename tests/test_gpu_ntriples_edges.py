"""The N-Triples loader on the device (ntriples.hip) at its kernel edges and at the grammar's terminals (nt_cases.py): 1 to 513 triple lines and
1 to 1025 distinct terms on either side of every block, wave and tile of its kernels, terms of 2 to 4100 bytes, every spelling of one term,
every layout of a line, refusals with their line numbers, first_id up to the last 32-bit id, typed literals at the bounds of each parser, the
recorded fixtures of the reference's parser suite and 2000 generated documents.  The device must equal nt_cases.reference — a parser written
from the grammar's productions that shares nothing with the device or with oracle.py (test_ntriples_cpu.py holds the oracle to it): the id
columns themselves, read in file order and mapped through decoded(), are the reference's triples as a sequence, duplicates included."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from oracle import oracle as orc
import nt_cases as nc


def from_device(torch, ptr, rows):
    if not rows:
        return np.zeros(0, np.uint32)

    class Col:
        __cuda_array_interface__ = {"shape": (rows,), "typestr": "<i4", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(Col(), device="cuda").cpu().numpy().view(np.uint32).copy()


def check_typed(decoded, typed, dec_hi):
    """the typed-value rows against oracle.ntriples_typed_value (int, Fraction): RDFGPU_TVF_NEEDS_HOST exactly where it allows it"""
    for t, (kind, lex, sfx) in enumerate(decoded):
        tag, lo, flags, hi, host = orc.ntriples_typed_value(kind, lex, sfx)
        row = typed[t]
        assert row["tag"] == tag, (lex, sfx, int(row["tag"]), tag)
        if host:
            assert row["flags"] & abi.TVF_NEEDS_HOST, (lex, sfx)
            continue
        assert not (row["flags"] & abi.TVF_NEEDS_HOST), (lex, sfx)
        if host is None:                                               # NaN: any payload
            assert np.isnan(np.array([row["lo"]], np.int64).view(np.float64)[0])
            continue
        assert (int(row["lo"]), int(row["flags"]), int(dec_hi[t])) == (lo, flags, hi), (lex, sfx, int(row["lo"]), lo, int(dec_hi[t]), hi)


def check_accepted(torch, text, want, first_id=1):
    """one parse: everything the handle hands out against the triples `want` (canonical terms, file order)"""
    data = text.encode("utf-8")
    nt = rf.NTriples(text, first_id=first_id)
    try:
        distinct = nc.distinct_terms(want)
        assert (nt.n_triples, nt.n_terms) == (len(want), len(distinct))
        decoded, typed, dec_hi = nt.decoded()
        assert len(decoded) == nt.n_terms and set(decoded) == distinct                  # (so: no term twice)
        cols = [from_device(torch, ptr, nt.n_triples) for ptr in nt.columns()]
        ids = np.concatenate(cols).astype(np.int64)
        assert np.array_equal(np.unique(ids), np.arange(first_id, first_id + nt.n_terms, dtype=np.int64))   # exactly these ids, every one used
        got = [tuple(decoded[int(i) - first_id] for i in row) for row in zip(*cols)]
        assert got == want                                                              # the sequence: file order, duplicates included
        terms = nt.terms()
        assert len(terms) == nt.n_terms and nt.term_bytes == sum(len(t) for t in terms)
        for t, d in zip(terms, decoded):
            assert orc.ntriples_decode_term(t) == d and t in data, (t, d)              # a spelling of this term, and one the text holds
        nl, ns = C.c_uint64(), C.c_uint64()
        assert nt._lib.rdfgpu_ntriples_decoded_info(nt._h, C.byref(nl), C.byref(ns)) == 0
        assert (nl.value, ns.value) == (sum(len(d[1]) for d in decoded), sum(len(d[2]) for d in decoded))
        check_typed(decoded, typed, dec_hi)
    finally:
        nt.close()


def check_refused(text, line):
    with pytest.raises(rf.RdfGpuError, match=r"triple line %d:" % line) as e:
        rf.NTriples(text)
    assert e.value.status == abi.ERR_INVALID, e.value


def check(torch, text, first_id=1):
    """the device against the reference; True when the text was accepted"""
    want = nc.reference(text)
    if isinstance(want, int):
        check_refused(text, want)
        return False
    check_accepted(torch, text, want, first_id)
    return True


@pytest.mark.parametrize("c", nc.ACCEPTED, ids=[c.name for c in nc.ACCEPTED])
def test_device_triples_equal_reference_in_file_order(torch_cuda, c):
    assert nc.reference(c.text) == c.want
    check_accepted(torch_cuda, c.text, c.want, c.first_id)


def test_refusals_carry_their_line_and_leave_the_loader_usable(torch_cuda):
    for c in nc.REFUSED:
        assert nc.reference(c.text) == c.want, c.name
        try:
            check_refused(c.text, c.want)
        except BaseException as e:
            raise AssertionError("%s: %r" % (c.name, c.text[:200])) from e
    check_accepted(torch_cuda, nc.GOOD + "\n", [nc.GOOD_WANT])                          # after the refusals, in the same process


def test_spellings_merge_and_the_escaped_datatype_is_typed(torch_cuda):
    """`"x"^^<…XMLSchema#strin\\u0067>` is the simple literal "x" (kind 3), `"12"^^<…intege\\u0072>` an xsd:integer."""
    c = nc.case_named("spellings")
    nt = rf.NTriples(c.text)
    decoded, typed, _ = nt.decoded()
    nt.close()
    assert nt.n_terms == nc.SPELLINGS_DISTINCT
    assert sum(d[1] == b"x" and d[0] in (nc.SIMPLE, nc.TYPED) for d in decoded) == 4     # "x", and x^^dt, x^^…strin, x^^…strings
    at = decoded.index((nc.TYPED, b"12", (nc.XSD + "integer").encode()))
    assert (int(typed[at]["tag"]), int(typed[at]["lo"])) == (abi.TV_INTEGER, 12)
    at = decoded.index((nc.SIMPLE, b"x", b""))
    assert int(typed[at]["tag"]) == abi.TV_STRING


def test_recorded_fixtures(torch_cuda):
    for g in nc.golden():
        assert nc.reference(g["text"]) == nc.golden_want(g), g["file"]
        assert check(torch_cuda, g["text"]) == ("triples" in g), g["file"]


def test_generated_documents(torch_cuda):
    """2000 parses, one call each; a good text is parsed after every refusal."""
    docs = nc.generated_documents()
    t0 = time.perf_counter()
    accepted = 0
    for k, d in enumerate(docs):
        try:
            ok = check(torch_cuda, d, first_id=1 + k % 7)
        except BaseException as e:
            raise AssertionError("document %d: %r" % (k, d)) from e
        accepted += ok
        if not ok and k % 16 == 1:
            check_accepted(torch_cuda, nc.GOOD + "\n", [nc.GOOD_WANT])
    print("generated documents: %d accepted, %d refused, %.1f s" % (accepted, len(docs) - accepted, time.perf_counter() - t0))
    assert accepted >= 400 and len(docs) - accepted >= 400


def test_first_id_up_to_the_last_object_id(torch_cuda):
    c = nc.case_named("terms-257")
    n_terms = len(nc.distinct_terms(c.want))
    last = 0xFFFFFFFF - n_terms                                                         # ids last .. 0xFFFFFFFE
    for first_id in (1, 5, last):
        check_accepted(torch_cuda, c.text, c.want, first_id)
    nt = rf.NTriples(c.text, first_id=last)
    ids = np.concatenate([from_device(torch_cuda, ptr, nt.n_triples) for ptr in nt.columns()])
    nt.close()
    assert int(ids.max()) == 0xFFFFFFFE and int(ids.min()) == last
    with pytest.raises(rf.RdfGpuError) as e:
        rf.NTriples(c.text, first_id=last + 1)
    assert e.value.status == abi.ERR_UNSUPPORTED, e.value
    with pytest.raises(rf.RdfGpuError) as e:
        rf.NTriples(c.text, first_id=0)
    assert e.value.status == abi.ERR_INVALID, e.value
    check_accepted(torch_cuda, c.text, c.want, 1)


def test_typed_literals_at_the_bounds_of_each_parser(torch_cuda):
    """check_accepted holds every row to oracle.ntriples_typed_value; here: the table's own expectation, literal by literal."""
    c = nc.case_named("typed-bounds")
    nt = rf.NTriples(c.text)
    decoded, typed, _ = nt.decoded()
    nt.close()
    for lex, name, expect in nc.TYPED_BOUNDS:
        row = typed[decoded.index((nc.TYPED, lex.encode(), (nc.XSD + name).encode()))]
        got = "host" if row["flags"] & abi.TVF_NEEDS_HOST else "null" if row["tag"] == abi.TV_NULL else "value"
        assert got == expect, (lex, name, got)
