"""Cases for the N-Triples loader (ntriples.hip) at its kernel edges and at the grammar's terminals, and an independent reference.

`reference(text)` is written from the productions of the N-Triples grammar (https://www.w3.org/TR/n-triples/#n-triples-grammar) with `re`
over the decoded text; it shares no code with oracle.py and none with the device's tokeniser.  Every case below is built from terms whose
canonical form is known by construction, so a case carries what it must parse to (`want`: the triples in file order, or the number of
the refused triple line) without asking any parser.  test_ntriples_cpu.py holds the reference and the oracle to `want`;
test_gpu_ntriples_edges.py holds the device to the reference.

Line structure is the project's (include/rdfgpu.h, section 7): lines end at LF, one CR directly before it (or before the end of the
text) belongs to the line end; blank lines and `#` lines are not counted; an error carries the 1-based number of the first bad line
among the counted ones."""
import json
import os
import random
import re
from collections import namedtuple

XSD = "http://www.w3.org/2001/XMLSchema#"
IRI, BNODE, SIMPLE, LANG, TYPED = 1, 2, 3, 4, 5                     # kinds of a canonical term (abi.NT_*)

# ---- the reference ------------------------------------------------------------------------------------------------------------------------
_HEX = r"[0-9A-Fa-f]"
_UCHAR = rf"\\u{_HEX}{{4}}|\\U{_HEX}{{8}}"
_ECHAR = r"""\\[tbnrf"'\\]"""
_IRIREF = rf"""<(?:[^\x00-\x20<>"{{}}|^`\\]|{_UCHAR})*>"""
_PN_CHARS_BASE = ("A-Za-z\u00C0-\u00D6\u00D8-\u00F6\u00F8-\u02FF\u0370-\u037D\u037F-\u1FFF\u200C-\u200D\u2070-\u218F\u2C00-\u2FEF"
                  "\u3001-\uD7FF\uF900-\uFDCF\uFDF0-\uFFFD\U00010000-\U000EFFFF")
_PN_CHARS_U = _PN_CHARS_BASE + "_:"
_PN_CHARS = _PN_CHARS_U + "\\-0-9\u00B7\u0300-\u036F\u203F-\u2040"
_BLANK_NODE_LABEL = rf"_:[{_PN_CHARS_U}0-9](?:[{_PN_CHARS}.]*[{_PN_CHARS}])?"
_LANGTAG = r"@[a-zA-Z]+(?:-[a-zA-Z0-9]+)*"
_STRING = rf"""\"(?:[^\x22\x5C\x0A\x0D]|{_ECHAR}|{_UCHAR})*\""""
_LITERAL = rf"{_STRING}(?:\^\^{_IRIREF}|{_LANGTAG})?"
_WS = r"[ \t]*"
_TRIPLE = re.compile(rf"{_WS}({_IRIREF}|{_BLANK_NODE_LABEL}){_WS}({_IRIREF}){_WS}({_IRIREF}|{_BLANK_NODE_LABEL}|{_LITERAL}){_WS}\.{_WS}(?:#.*)?")
_LITERAL_PARTS = re.compile(rf"({_STRING})(?:\^\^({_IRIREF})|({_LANGTAG}))?")
_ESCAPE = re.compile(rf"""({_UCHAR})|\\([tbnrf"'\\])""")
_ECHAR_VALUE = {"t": "\t", "b": "\b", "n": "\n", "r": "\r", "f": "\f", '"': '"', "'": "'", "\\": "\\"}


class Refused(Exception):
    pass


def _unescape(s):
    def one(m):
        if m.group(2) is not None:
            return _ECHAR_VALUE[m.group(2)]
        cp = int(m.group(1)[2:], 16)
        if cp > 0x10FFFF or 0xD800 <= cp <= 0xDFFF:                  # a UCHAR names a Unicode scalar value
            raise Refused
        return chr(cp)
    return _ESCAPE.sub(one, s).encode("utf-8")


def canonical(term):
    """One term as the grammar matched it -> (kind, lexical bytes, suffix bytes): escapes decoded, the language tag in lower case, the
    datatype IRI decoded, a decoded xsd:string datatype = the simple literal."""
    if term[0] == "<":
        return IRI, _unescape(term[1:-1]), b""
    if term[0] == "_":
        return BNODE, term[2:].encode("utf-8"), b""
    string, datatype, lang = _LITERAL_PARTS.fullmatch(term).groups()
    lex = _unescape(string[1:-1])
    if lang is not None:
        return LANG, lex, lang[1:].lower().encode("ascii")
    if datatype is not None:
        dt = _unescape(datatype[1:-1])
        if dt != (XSD + "string").encode("ascii"):
            return TYPED, lex, dt
    return SIMPLE, lex, b""


def reference(text):
    """The triples of `text` in file order, each three canonical terms — or, on refusal, the number (an int) of the first bad triple line."""
    if isinstance(text, bytes):
        text = text.decode("utf-8")
    out, counted = [], 0
    for line in text.split("\n"):
        if line.endswith("\r"):
            line = line[:-1]
        body = line.lstrip(" \t")
        if not body or body[0] == "#":
            continue
        counted += 1
        m = _TRIPLE.fullmatch(line)
        if m is None:
            return counted
        try:
            out.append(tuple(canonical(t) for t in m.groups()))
        except Refused:
            return counted
    return out


# ---- terms known by construction: (as written, canonical) ----------------------------------------------------------------------------------
Term = namedtuple("Term", "text canon")


def iri(s, written=None):
    return Term("<%s>" % (s if written is None else written), (IRI, s.encode("utf-8"), b""))


def bnode(label):
    return Term("_:" + label, (BNODE, label.encode("utf-8"), b""))


def lit(lex, written=None, lang=None, dt=None, dt_written=None):
    """`lex` is the decoded lexical form; `written` its spelling between the quotes when that differs; `dt` the decoded datatype IRI."""
    w = '"%s"' % (lex if written is None else written)
    lexb = lex.encode("utf-8")
    if lang is not None:
        return Term(w + "@" + lang, (LANG, lexb, lang.lower().encode("ascii")))
    if dt is not None:
        w += "^^<%s>" % (dt if dt_written is None else dt_written)
        return Term(w, (SIMPLE, lexb, b"") if dt == XSD + "string" else (TYPED, lexb, dt.encode("utf-8")))
    return Term(w, (SIMPLE, lexb, b""))


def uchar(s, big=False):
    return "".join(("\\U%08X" if big or ord(c) > 0xFFFF else "\\u%04X") % ord(c) for c in s)


Case = namedtuple("Case", "name text want first_id")


def case(name, text, want, first_id=1):
    return Case(name, text, want, first_id)


def document(triples, sep=" ", dot=" .", eol="\n", last_eol=True, between=None):
    """Text and expected triples of a list of (s, p, o) Terms; `between` = a line put between every two triples."""
    lines = [sep.join(t.text for t in tr) + dot for tr in triples]
    if between is not None:
        lines = [x for l in lines for x in (l, between)][:-1]
    text = eol.join(lines) + (eol if last_eol else "")
    return text, [tuple(t.canon for t in tr) for tr in triples]


S, P, O = iri("http://e/s"), iri("http://e/p"), iri("http://e/o")
GOOD = "%s %s %s ." % (S.text, P.text, O.text)
GOOD_WANT = (S.canon, P.canon, O.canon)


# ---- line and occurrence counts: nt_terms runs 256 lines a block, nt_unique / nt_assign 256 of the 3 L occurrences --------------------------------
LINE_COUNTS = [1, 85, 86, 255, 256, 257, 513]


def _lines_case(n):
    subj = [iri("http://e/s%d" % i) for i in range(7)] + [bnode("b%d" % i) for i in range(3)]
    pred = [iri("http://e/p%d" % i) for i in range(3)]
    obj = [lit("v%d" % i) for i in range(11)] + subj[:5]
    return case("lines-%d" % n, *document([(subj[i % 10], pred[i % 3], obj[(i * 5) % 16]) for i in range(n)]))


# ---- distinct-term counts: nt_term_bytes gives a wave 16 terms and a block 64, the decode kernels a block 256 ------------------------------------
TERM_COUNTS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025]


def _terms_case(n):
    if n == 1:
        t = iri("http://e/only")
        return case("terms-1", *document([(t, t, t)] * 300))
    n_lit = n // 3
    iris = [iri("http://e/t%d" % i) if i % 4 else bnode("n%d" % i) for i in range(n - n_lit)]
    preds = [t for t in iris if t.canon[0] == IRI]
    lits = [(lit("w%d" % i), lit("w%d" % i, lang="en"), lit(str(i), dt=XSD + "integer"))[i % 3] for i in range(n_lit)]
    return case("terms-%d" % n, *document([(iris[i], preds[(i * 7 + 1) % len(preds)], lits[i % n_lit]) for i in range(len(iris))]))


def _all_distinct_case():
    rows = [(iri("http://e/a%d" % i) if i % 5 else bnode("a%d" % i), iri("http://e/q%d" % i), lit("o%d" % i) if i % 2 else iri("http://e/o%d" % i))
            for i in range(100)]
    return case("all-distinct-300", *document(rows))


# ---- term lengths as written: the 64-lane stride of nt_term_bytes, the byte-compare loop of nt_unique, the offset scans -------------------------
WRITTEN_LENGTHS = [2, 63, 64, 65, 127, 128, 129, 4100]


def _iri_of_length(n, tag):
    return iri("") if n == 2 else iri("http://e/%s" % tag + "x" * (n - 2 - len("http://e/%s" % tag)))


def _lit_of_length(n, tag):
    return lit(tag + "y" * (n - 2 - len(tag)))


def _lengths_case():
    rows = []
    for n in WRITTEN_LENGTHS:
        a, b = _iri_of_length(n, "i"), (_lit_of_length(n, "l") if n > 2 else lit(""))
        rows += [(a, P, b), (S, P, a), (a, P, O)]
    e100 = "\u00e9" * 100
    decoded_differs = [lit(e100, written=uchar(e100)), iri("http://e/" + e100, written="http://e/" + uchar(e100)), lit("\U0001F600", written="\\U0001F600"),
                       lit("\t\b\n\r\f\"'\\", written="\\t\\b\\n\\r\\f\\\"\\'\\\\"), lit(e100), iri("http://e/" + e100)]
    for t in decoded_differs:
        rows.append((t if t.canon[0] == IRI else S, P, t))
    # long terms in two spellings, several hundred lines apart: they must merge
    long_lex = "z" * 4098
    long_a, long_b = lit(long_lex), lit(long_lex, written="\\u007A" + long_lex[1:])
    iri_a, iri_b = _iri_of_length(129, "m"), None
    iri_b = iri(iri_a.canon[1].decode(), written=iri_a.canon[1].decode()[:-1] + "\\U00000078")
    filler = [(iri("http://e/f%d" % (i % 37)), P, lit("f%d" % (i % 53))) for i in range(400)]
    rows = [(iri_a, P, long_a)] + rows + filler + [(iri_b, P, long_b), (S, P, long_a)]
    return case("written-lengths", *document(rows))


# ---- spellings of one term ------------------------------------------------------------------------------------------------------------------
def _spellings_case():
    objs = [
        # the spellings test_gpu_parity.py already holds
        lit("aA\n", written="aA\\n"), lit("aA\n", written="a\\u0041\\n"), lit("aA\n", written="\\u0061\\U00000041\\u000A"),
        lit("x"), lit("x", dt=XSD + "string"), lit("v", lang="en-GB"), lit("v", lang="EN-gb"), lit("v", lang="en-gb"),
        iri("http://example.org/caf\u00e9", written="http://example.org/caf\\u00E9"), iri("http://example.org/caf\u00e9"),
        lit("x", dt="http://example.org/dt"), lit("x", dt="http://example.org/dt", dt_written="http://example.org/d\\u0074"),
        # a datatype IRI with UCHAR escapes: xsd:string in three spellings = the simple literal; xsd:integer is typed as an integer
        lit("x", dt=XSD + "string", dt_written=XSD + "strin\\u0067"), lit("x", dt=XSD + "string", dt_written="\\u0068ttp" + XSD[4:] + "string"),
        lit("x", dt=XSD + "string", dt_written=uchar(XSD + "string", big=True)),
        lit("x", dt=XSD + "strin"), lit("x", dt=XSD + "strings"), lit("x", dt=XSD + "strings", dt_written=XSD + "string\\u0073"),
        lit("12", dt=XSD + "integer", dt_written=XSD + "intege\\u0072"), lit("12", dt=XSD + "integer"),
        # one label as a blank node, an IRI and a literal: three terms
        bnode("x"), iri("x"), lit("x"),
        # a language tag against a datatype of the same letters: two terms
        lit("a", lang="en"), lit("a", dt="en"),
    ]
    rows = [(S if o.canon[0] != BNODE else o, P, o) for o in objs]
    rows += [(objs[8], P, O), (objs[9], objs[9], objs[9])]
    return case("spellings", *document(rows))


SPELLINGS_DISTINCT = 3 + 12                                         # S, P, O and: aA\n, x, v@en-gb, café, x^^dt, x^^strin, x^^strings, 12^^integer, _:x, <x>, a@en, a^^en


# ---- layout ---------------------------------------------------------------------------------------------------------------------------------
def _layout_cases():
    b, xl, xe = bnode("b"), lit("x"), lit("x", lang="en")
    two, two_want = document([(S, P, O), (b, P, xl)])
    cs = [
        case("no-final-newline", *document([(S, P, O), (b, P, xl)], last_eol=False)),
        case("crlf", *document([(S, P, O), (b, P, xe), (S, P, b)], eol="\r\n")),
        case("crlf-no-final-newline", "%s\r\n\r\n# c\r\n \t\r\n%s\r" % (GOOD, GOOD), [GOOD_WANT] * 2),
        case("tabs-and-spaces", " \t%s\t%s   %s\t.\t \n\t%s \t.  \n" % (S.text, P.text, O.text, "\t \t".join(t.text for t in (b, P, xe))),
             [GOOD_WANT, (b.canon, P.canon, xe.canon)]),
        case("no-white-space", "".join("%s%s%s.\n" % (s_.text, P.text, o_.text) for s_, o_ in ((S, O), (S, xl), (S, xe), (b, O))),
             [GOOD_WANT, (S.canon, P.canon, xl.canon), (S.canon, P.canon, xe.canon), (b.canon, P.canon, O.canon)]),
        case("dot-comment", "%s %s %s .# c\n%s %s _:b.\n%s %s _:b.# c\n%s %s _:a.b .\n%s %s _:a.b.\n" % ((S.text, P.text, O.text) + (S.text, P.text) * 4),
             [GOOD_WANT, (S.canon, P.canon, b.canon), (S.canon, P.canon, b.canon), (S.canon, P.canon, bnode("a.b").canon), (S.canon, P.canon, bnode("a.b").canon)]),
        case("label-then-iri", "_:b%s %s .\n_:b-1:c.d%s%s.\n" % (P.text, O.text, P.text, O.text), [(b.canon, P.canon, O.canon), (bnode("b-1:c.d").canon, P.canon, O.canon)]),
        case("labels", *document([(bnode("1"), P, bnode("_")), (bnode(":"), P, bnode("0a-")), (bnode("\u00e9\u65e5"), P, bnode("a\u00b7b"))])),
        case("empty-text", "", []),
        case("comment-only", "# c\n  # d\n\n\t#\n", []),
        case("white-space-only", " \t \n\n   \n\t", []),
        case("comment-between", *document([(S, P, O), (b, P, xl), (S, P, xe), (S, P, b)], between="# <a> <b> <c> .")),
        case("last-line-of-blanks", two + "  \t ", two_want),
        case("comment-without-newline", two + "# end", two_want),
        # what stays outside the terminals and is accepted: relative IRIs, subtags of any length, a UCHAR that decodes to a character no IRI may hold
        case("outside-accepted", *document([(iri("a"), iri("b"), iri("")), (S, P, lit("x", lang="abcdefghijklmnop-123456789")),
                                            (S, P, iri("http://e/a b", written="http://e/a\\u0020b"))])),
    ]
    return cs


# ---- refusals, each with its line number -----------------------------------------------------------------------------------------------------
GRAMMAR_REFUSALS = [                                                 # accepted before the terminals were enforced
    "_: <p> <o> .", "_:-a <p> <o> .", "_:` <p> <o> .", "_:a. <p> <o> .", "<s> <p> _:b..", "<s> _:p <o> .",
    '<s> <p> "x"@ .', '<s> <p> "x"@- .', '<s> <p> "x"@en- .', '<s> <p> "x"@1en .',
    "<s> <http:// /p> <o> .", "<s> <http://a<b> <o> .", '<s> <http://a"b> <o> .', "<s> <http://a{b> <o> .",
    '<s> <p> "a\rb" .',
]
MORE_REFUSALS = [
    "<s> <http://a}b> <o> .", "<s> <p> <http://a|b> .", "<http://a^b> <p> <o> .", "<s> <p> <http://a`b> .", "<s> <p> <a\tb> .", "<s> <p> <a\x01b> .",
    '<s> <p> "x"^^<http://a b> .', '<s> <p> "x"^^<a"b> .', '<s> <p> "x"^^ <d> .', '<s> <p> "x"@en^^<d> .', '<s> <p> "x"@en-a- .', '<s> <p> "x"@-en .',
    "<s> <p> _:.a .", "<s> <p> _:", "<s> <p> _:a .b .", "_:a _:b _:c .", "<s> <p> <o> . <s> <p> <o> .", "\ufeff<s> <p> <o> .",
    '<s> <p> "a\\', '<s> <p> "\\uD800" .', "<a\\u00e> <p> <o> .", '<s> <p> "x"^^<\\uDFFF> .', "<s> <p> <o> ,", "<s> <p> <o> . x", "<s> <p> <o> .\f",
]
EXISTING_REFUSALS = [                                                # the bad lines of test_gpu_parity.py
    ("<a> <b> <c> .\n<a> <b> .\n", 2), ('<a> <b> "open\n', 1), ("<a> <b> <c> <d> .\n", 1), ('"lit" <b> <c> .\n', 1), ("<a> <b> <c>\n", 1),
    ('<a> <b> "bad \\q escape" .\n', 1), ('<a> <b> "\\u12" .\n', 1), ('<a> <b> "\\uD800" .\n', 1), ("<a\\n> <b> <c> .\n", 1), ('<a> <b> "\\U00110000" .\n', 1),
]


def _bad_line_in_600(at, second=None):
    """600 triple lines, `at` (1-based, counted) bad; 40 blank or comment lines before it do not count."""
    lines = []
    for i in range(1, 601):
        if i == at:
            lines += ["", "# not a line", "   ", "\t# nor this"] * 10
        lines.append("<s> _:p <o> ." if i in (at, second) else "<http://e/s%d> <http://e/p> \"%d\" ." % (i % 50, i))
    return "\n".join(lines) + "\n"


def _refusal_cases():
    cs = []
    for i, bad in enumerate(GRAMMAR_REFUSALS + MORE_REFUSALS):
        line = 1 + i % 3                                             # the bad line first, second or third; a comment and a blank line do not count
        text = "".join(GOOD + "\n" for _ in range(line - 1)) + "# c\n\n" + bad + "\n" + GOOD + "\n"
        cs.append(case("refused-%02d" % i, text, line))
    cs += [case("refused-existing-%d" % i, t, n) for i, (t, n) in enumerate(EXISTING_REFUSALS)]
    cs.append(case("refused-cr-only-file", GOOD + "\r" + GOOD + "\r", 1))
    cs += [case("refused-line-%d-of-600" % at, _bad_line_in_600(at), at) for at in (1, 256, 257, 600)]
    cs.append(case("refused-two-bad-lines", _bad_line_in_600(300, 258), 258))
    cs.append(case("refused-two-bad-lines-one-block", "%s\n<s> <p> <o>\n%s\n_: <p> <o> .\n" % (GOOD, GOOD), 2))
    return cs


# ---- typed literals at the bounds of each parser: (lexical form, datatype, what oracle.ntriples_typed_value must say) -----------------------------
# "value" = typed on the device, "null" = the lexical form is invalid (RDFGPU_TV_NULL), "host" = RDFGPU_TVF_NEEDS_HOST
DEC_MAX = "170141183460469231731.687303715884105727"
TYPED_BOUNDS = [
    ("9223372036854775807", "integer", "value"), ("9223372036854775808", "integer", "null"), ("-9223372036854775807", "long", "value"),
    ("-9223372036854775808", "integer", "value"), ("-9223372036854775809", "integer", "null"),
    ("2147483647", "int", "value"), ("2147483648", "int", "null"), ("-2147483647", "int", "value"), ("-2147483648", "int", "value"), ("-2147483649", "int", "null"),
    ("1234567890123456789012345", "integer", "null"), ("+", "integer", "null"), ("-", "int", "null"), ("+-1", "integer", "null"),
    (DEC_MAX, "decimal", "value"), (DEC_MAX[:-1] + "8", "decimal", "null"), ("-" + DEC_MAX[:-1] + "8", "decimal", "value"), ("-" + DEC_MAX[:-1] + "9", "decimal", "null"),
    ("0.123456789012345678", "decimal", "value"), ("0.1234567890123456789", "decimal", "null"), ("0.1234567890123456780", "decimal", "value"),
    (".0", "decimal", "value"), ("-.", "decimal", "null"), ("+.5", "decimal", "value"),
    ("9007199254740991", "double", "value"), ("9007199254740992", "double", "host"),
    ("1e22", "double", "value"), ("1e23", "double", "host"), ("1e-22", "double", "value"), ("1e-23", "double", "host"),
    ("1.5e23", "double", "value"), ("1.5e24", "double", "host"), ("0." + "0" * 21 + "1", "double", "value"), ("0." + "0" * 22 + "1", "double", "host"),
    ("1234567890123456789", "double", "host"), ("12345678901234567890", "double", "host"), ("0.000123456789012345", "double", "value"),
    ("0e10000", "double", "value"), ("0e10001", "double", "host"),
    ("+inf", "double", "value"), ("-INF", "double", "value"), ("+nan", "double", "host"), ("1e", "double", "host"), (".e5", "double", "host"), ("1.", "double", "value"),
    ("16777215", "float", "value"), ("16777216", "float", "host"),
    ("1e10", "float", "value"), ("1e11", "float", "host"), ("1e-10", "float", "value"), ("1e-11", "float", "host"), ("2.5e11", "float", "value"), ("2.5e12", "float", "host"),
    ("+inf", "float", "value"), ("+nan", "float", "host"),
]


def _typed_case():
    return case("typed-bounds", *document([(S, iri("http://e/p%d" % (i % 5)), lit(lex, dt=XSD + name)) for i, (lex, name, _) in enumerate(TYPED_BOUNDS)]))


# ---- the recorded outcomes of the reference's parser fixtures --------------------------------------------------------------------------------
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ntriples_kats.json"), encoding="utf-8") as f:
        return json.load(f)["fixtures"]


def golden_want(g):
    """A recorded outcome in the form `reference` returns."""
    if "refused_line" in g:
        return g["refused_line"]
    return [tuple((k, lex.encode("utf-8"), sfx.encode("utf-8")) for k, lex, sfx in tr) for tr in g["triples"]]


# ---- a seeded differential generator ---------------------------------------------------------------------------------------------------------
N_GENERATED = 2000
MUTATION_BYTES = "<>\"_:.@^\\# \t-a7"


def _gen_chars(rng, alphabet, lo, hi, escapes):
    out = []
    for _ in range(rng.randint(lo, hi)):
        r = rng.random()
        if r < 0.08:
            out.append(uchar(rng.choice("abcxyzABZ"), big=rng.random() < 0.4))
        elif r < 0.14 and escapes:
            out.append(rng.choice(["\\t", "\\n", "\\\"", "\\\\", "\\'", "\\r", "\\b", "\\f"]))
        else:
            out.append(rng.choice(alphabet))
    return "".join(out)


def _gen_iri(rng):
    if rng.random() < 0.3:
        return rng.choice(["<http://e/s>", "<http://e/p>", "<a>", "<>", "<%sstring>" % XSD, "<%sinteger>" % XSD])
    return "<" + _gen_chars(rng, "abcpq019:/.#-_~?=\u00e9\u65e5", 0, 12, False) + ">"


def _gen_bnode(rng):
    first = rng.choice("abz09_:\u00e9")
    rest = _gen_chars(rng, "ab01-._:\u00e9\u65e5", 0, 6, False).replace("\\", "")       # (no escapes in a label: the letters of one that was drawn stay)
    rest = rest.rstrip(".")
    return "_:" + first + rest


def _gen_literal(rng):
    s = '"' + _gen_chars(rng, "abc xyz019.<>#@^_:-'\t\u00e9\u65e5", 0, 10, True) + '"'
    r = rng.random()
    if r < 0.25:
        s += "@" + rng.choice(["en", "EN", "fr-CA", "de-1996", "x-a-b-c", "zh-Hant-TW"])
    elif r < 0.5:
        s += "^^" + _gen_iri(rng)
    return s


def _gen_line(rng):
    r = rng.random()
    if r < 0.06:
        return rng.choice(["", "   ", "# comment <a> <b> <c> .", "\t# c"])
    s_ = _gen_bnode(rng) if rng.random() < 0.3 else _gen_iri(rng)
    o_ = [_gen_iri, _gen_bnode, _gen_literal][rng.randrange(3)](rng)
    ws = lambda: rng.choice(["", " ", " ", " ", "\t", "  \t "])
    line = ws() + s_ + ws() + _gen_iri(rng) + ws() + o_ + ws() + "." + ws()
    if rng.random() < 0.15:
        line += "# " + _gen_chars(rng, "abc <>.\"", 0, 6, False)
    return line


def generated_documents():
    """2000 documents of 1 to 6 lines drawn from the grammar (ASCII plus `é` and `日`, UCHAR escapes of letters only); every second one gets one
    character inserted, deleted or replaced.  No CR anywhere.  Deterministic."""
    rng = random.Random(20250611)
    docs = []
    for d in range(N_GENERATED):
        text = "\n".join(_gen_line(rng) for _ in range(rng.randint(1, 6))) + ("\n" if rng.random() < 0.8 else "")
        if d % 2:
            at, how, c = rng.randrange(len(text) + 1), rng.randrange(3), rng.choice(MUTATION_BYTES)
            if how == 0 or at == len(text):
                text = text[:at] + c + text[at:]
            elif how == 1:
                text = text[:at] + text[at + 1:]
            else:
                text = text[:at] + c + text[at + 1:]
        docs.append(text)
    return docs


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------
ACCEPTED = ([_lines_case(n) for n in LINE_COUNTS] + [_terms_case(n) for n in TERM_COUNTS] +
            [_all_distinct_case(), _lengths_case(), _spellings_case(), _typed_case()] + _layout_cases())
REFUSED = _refusal_cases()
CASES = ACCEPTED + REFUSED
CASE_IDS = [c.name for c in CASES]


def case_named(name):
    return next(c for c in CASES if c.name == name)


def distinct_terms(want):
    return {t for tr in want for t in tr}
