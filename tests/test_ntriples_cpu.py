"""The N-Triples cases (nt_cases.py) on the CPU: the independent reference written from the grammar's productions and the oracle's
restatement of the device's loader (oracle.ntriples_encode + ntriples_decode_term) agree — the same refusal on the same triple line, or the
same canonical triples in file order — on every case, on every recorded fixture of the reference's parser suite and on 2000 generated
documents; both give what each case was built to give; and the tables hold the counts and lengths they are there for."""
import pytest

from oracle import oracle as orc
from rdf_fusion_amd import abi
import nt_cases as nc


def oracle_outcome(text):
    """oracle.ntriples_encode in the form nt_cases.reference returns: canonical triples in file order, or the refused line."""
    try:
        terms, s, p, o = orc.ntriples_encode(text)
    except ValueError as e:
        return e.args[0]
    canon = [orc.ntriples_decode_term(t) for t in terms]
    return [(canon[a - 1], canon[b - 1], canon[c - 1]) for a, b, c in zip(s, p, o)]


@pytest.mark.parametrize("c", nc.CASES, ids=nc.CASE_IDS)
def test_reference_and_oracle_give_what_the_case_was_built_for(c):
    assert nc.reference(c.text) == c.want
    assert oracle_outcome(c.text) == c.want


def test_recorded_fixtures():
    fixtures = nc.golden()
    assert len(fixtures) == 12 and sum("refused_line" in g for g in fixtures) == 6
    for g in fixtures:
        assert nc.reference(g["text"]) == nc.golden_want(g), g["file"]
        assert oracle_outcome(g["text"]) == nc.golden_want(g), g["file"]


def test_generated_documents():
    docs = nc.generated_documents()
    assert len(docs) == nc.N_GENERATED and len(set(docs)) > 1900 and not any("\r" in d for d in docs)
    assert all(1 <= len(d.split("\n")) <= 7 for d in docs[::2])                    # unmutated: 1 to 6 lines (and what follows the last LF)
    outcomes = [nc.reference(d) for d in docs]
    refused = sum(isinstance(r, int) for r in outcomes)
    assert refused >= 400 and len(docs) - refused >= 400, refused
    assert all(isinstance(r, list) for r in outcomes[::2])                         # drawn from the grammar: accepted before mutation
    assert sum(isinstance(r, list) and len(r) > 0 for r in outcomes[1::2]) >= 100    # a mutation that still parses, and one that does not
    for d, r in zip(docs, outcomes):
        assert oracle_outcome(d) == r, d


def test_tables_hold_their_edges():
    for n in nc.LINE_COUNTS:
        c = nc.case_named("lines-%d" % n)
        assert len(c.want) == n and len(nc.distinct_terms(c.want)) == (24 if n > 1 else 3)   # 10 subjects, 3 predicates, 11 literals
    assert [3 * n for n in (85, 86)] == [255, 258] and {255, 256, 257, 513} <= set(nc.LINE_COUNTS)   # either side of a block of lines / of occurrences
    for n in nc.TERM_COUNTS:
        c = nc.case_named("terms-%d" % n)
        assert len(nc.distinct_terms(c.want)) == n, n
    one = nc.case_named("terms-1")
    assert len(one.want) == 300 and len(set(one.want)) == 1 and len(set(one.want[0])) == 1
    assert max(len(c.want) for c in nc.ACCEPTED) <= 1100
    alld = nc.case_named("all-distinct-300")
    assert len(alld.want) == 100 and len(nc.distinct_terms(alld.want)) == 300
    # written lengths: every length occurs as an IRI and (above 2) as a literal; decoded lengths that differ; two spellings far apart
    c = nc.case_named("written-lengths")
    written = {}
    for line in c.text.split("\n"):
        for tok in line.split(" ")[:3]:
            written.setdefault(len(tok.encode("utf-8")), set()).add(tok[:1])
    for n in nc.WRITTEN_LENGTHS:
        assert written[n] >= ({"<", '"'} if n > 2 else {"<"}), n
    assert "<>" in c.text and {(nc.SIMPLE, b""), (nc.IRI, b"")} <= {t[:2] for t in nc.distinct_terms(c.want)}
    e100 = ("é" * 100).encode("utf-8")
    terms = nc.distinct_terms(c.want)
    assert {(nc.SIMPLE, e100, b""), (nc.IRI, b"http://e/" + e100, b""), (nc.SIMPLE, "\U0001F600".encode("utf-8"), b""), (nc.SIMPLE, b"\t\b\n\r\f\"'\\", b"")} <= terms
    assert c.text.count("\\u00E9") == 300 and "\\U0001F600" in c.text and '"\\t\\b\\n\\r\\f\\"\\\'\\\\"' in c.text
    long_lit = (nc.SIMPLE, b"z" * 4098, b"")
    at = [i for i, tr in enumerate(c.want) if tr[2] == long_lit]
    assert len(at) == 3 and at[1] - at[0] > 400 and c.text.count('"' + "z" * 4098 + '"') == 2 and c.text.count('"\\u007A' + "z" * 4097 + '"') == 1
    long_iri = [i for i, tr in enumerate(c.want) if tr[0][0] == nc.IRI and len(tr[0][1]) == 127 and tr[0][1].startswith(b"http://e/m")]
    assert len(long_iri) == 2 and long_iri[1] - long_iri[0] > 400 and "\\U00000078>" in c.text
    # spellings: the distinct terms by construction
    c = nc.case_named("spellings")
    terms = nc.distinct_terms(c.want)
    assert len(terms) == nc.SPELLINGS_DISTINCT
    assert {(nc.SIMPLE, b"x", b""), (nc.IRI, b"x", b""), (nc.BNODE, b"x", b""), (nc.LANG, b"a", b"en"), (nc.TYPED, b"a", b"en"),
            (nc.TYPED, b"x", (nc.XSD + "strin").encode()), (nc.TYPED, b"x", (nc.XSD + "strings").encode()), (nc.TYPED, b"12", (nc.XSD + "integer").encode())} <= terms
    assert c.text.count("strin\\u0067>") == 1 and c.text.count("intege\\u0072>") == 1 and "\\U00000068\\U00000074" in c.text
    assert orc.ntriples_typed_value(nc.TYPED, b"12", (nc.XSD + "integer").encode())[0] == abi.TV_INTEGER
    # refusals: every listed line is there, and the bad line of the long documents sits past a block of lines
    assert len(nc.REFUSED) == len(nc.GRAMMAR_REFUSALS) + len(nc.MORE_REFUSALS) + len(nc.EXISTING_REFUSALS) + 7
    assert {c.want for c in nc.REFUSED} >= {1, 2, 3, 256, 257, 258, 600}
    assert all(isinstance(c.want, int) for c in nc.REFUSED) and all(isinstance(c.want, list) for c in nc.ACCEPTED)
    assert len(set(nc.CASE_IDS)) == len(nc.CASES)


def test_typed_bounds_are_what_the_table_says():
    """oracle.ntriples_typed_value (int, Fraction: nothing shared with the device) classifies every literal of the table as the table says."""
    null, host = 0, 0
    for lex, name, expect in nc.TYPED_BOUNDS:
        tag, lo, flags, hi, needs_host = orc.ntriples_typed_value(nc.TYPED, lex.encode(), (nc.XSD + name).encode())
        got = "host" if needs_host else "null" if tag == abi.TV_NULL else "value"
        assert got == expect, (lex, name, got)
        assert bool(flags & abi.TVF_NEEDS_HOST) == (expect == "host")
        null += expect == "null"
        host += expect == "host"
    assert null >= 10 and host >= 15
    c = nc.case_named("typed-bounds")
    assert len(nc.distinct_terms(c.want)) == len(nc.TYPED_BOUNDS) + 1 + 5
