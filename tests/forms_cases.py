"""Shared cases of the functional forms (IF, COALESCE, IN / NOT IN), the term tests (isIRI, isBlank, isLiteral, isNumeric), LANG(x) = "tag"
and the LeftMark join, with Python references that share nothing with the device code or with oracle/.

A typed value is a tuple (tag, payload); the error value is NULL = (TV_NULL, None).  Payloads: IRI / blank node: the rank; string: (rank,
language id, is empty); boolean: bool; float / double: the IEEE bits; decimal: the value * 10^18; int / integer: the value; dateTime / time /
date: (timeline seconds * 10^18, has a timezone); duration: an opaque number; other literal: (lexical id, datatype id).  A native boolean
(what EBV / AND / OR / NOT work on) is 0, 1 or 2 = null; an object id is an int, 0 = unbound.

The references restate, line by line:
  IF            lib/functions/src/scalar/functional_form/sparql_if.rs:50-57 over Boolean::try_from (lib/model/src/xsd/boolean.rs:93-102)
  COALESCE      DataFusion's coalesce (lib/functions/src/registry.rs:264-270): the first argument that is not null
  isIRI ..      lib/functions/src/scalar/terms/is_{iri,blank,literal,numeric}.rs (the null value: ThinError::expected)
  IN / NOT IN   lib/execution/src/sparql/rewriting/expression_rewriter.rs:302-322 (rewrite_in) and :105-107
  LANG(x) = t   lib/functions/src/scalar/terms/lang.rs:49-55 under `=`
  `=`           PartialOrd for TypedValueRef, lib/model/src/typed_value.rs:162-261 (what IN compares with)
  EBV           lib/functions/src/builtin/native/effective_boolean_value.rs:99-119
  LeftMark      DataFusion's JoinType::LeftMark: every left row once, with "some right row equals it on every key and passes the filter"
"""
import struct

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.engine import TV_DTYPE

E18 = 10 ** 18
NULL = (abi.TV_NULL, None)
NUMERIC = (abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE)
TIMESTAMPS = (abi.TV_DATE_TIME, abi.TV_TIME, abi.TV_DATE)


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f32_of(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def f64_of(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


# ---------------------------------------------------------------------------------------------------
# the typed-value table: at least one id of every tag; id 0 is null, BEYOND lies outside the table
# ---------------------------------------------------------------------------------------------------
LANGUAGE_TAGS = ["", "en", "de", "en-GB"]          # language id -> tag (id 0: no language)
F32_NAN, F64_NAN = 0x7FC00000, 0x7FF8000000000000
TABLE = [
    NULL,                                           # 0
    (abi.TV_NAMED_NODE, 1),                         # 1
    (abi.TV_NAMED_NODE, 2),                         # 2
    (abi.TV_BLANK_NODE, 1),                         # 3
    (abi.TV_STRING, (5, 0, False)),                 # 4  a simple string
    (abi.TV_STRING, (5, 1, False)),                 # 5  the same rank @en
    (abi.TV_STRING, (6, 2, False)),                 # 6  @de
    (abi.TV_STRING, (0, 0, True)),                  # 7  ""
    (abi.TV_BOOLEAN, True),                         # 8
    (abi.TV_BOOLEAN, False),                        # 9
    (abi.TV_FLOAT, F32_NAN),                        # 10
    (abi.TV_FLOAT, f32_bits(0.0)),                  # 11
    (abi.TV_FLOAT, f32_bits(-0.0)),                 # 12
    (abi.TV_FLOAT, f32_bits(1.5)),                  # 13
    (abi.TV_DOUBLE, f64_bits(2.5)),                 # 14
    (abi.TV_DOUBLE, F64_NAN),                       # 15
    (abi.TV_DOUBLE, f64_bits(-7.0)),                # 16
    (abi.TV_DECIMAL, 25 * E18 // 10),               # 17 2.5 (the side table)
    (abi.TV_DECIMAL, -3 * E18),                     # 18
    (abi.TV_INT, 1),                                # 19
    (abi.TV_INT, -5),                               # 20
    (abi.TV_INT, -2 ** 31),                         # 21 ABS overflows
    (abi.TV_INTEGER, 1),                            # 22
    (abi.TV_INTEGER, 7),                            # 23
    (abi.TV_INTEGER, 0),                            # 24
    (abi.TV_INTEGER, -2 ** 63),                     # 25 ABS overflows
    (abi.TV_DATE_TIME, (1700000000 * E18, True)),   # 26
    (abi.TV_TIME, (3600 * E18, True)),              # 27
    (abi.TV_DATE, (1700006400 * E18, False)),       # 28
    (abi.TV_DURATION, 3),                           # 29
    (abi.TV_OTHER, (1, 1)),                         # 30
    (abi.TV_OTHER, (2, 1)),                         # 31
    (abi.TV_STRING, (7, 3, False)),                 # 32 @en-GB
    (abi.TV_STRING, (8, 0, False)),                 # 33 the simple string "-nan": xsd:float of it is a refusal of the device, not a value
]
N_IDS = len(TABLE)
BEYOND = N_IDS + 6                                  # an id beyond the table: ENC_TV gives the null value
ID = {"null": 0, "iri": 1, "iri2": 2, "blank": 3, "str": 4, "str_en": 5, "str_de": 6, "str_empty": 7, "true": 8, "false": 9, "f32_nan": 10,
      "f32_pos0": 11, "f32_neg0": 12, "f32": 13, "f64": 14, "f64_nan": 15, "f64_neg": 16, "dec": 17, "dec_neg": 18, "int1": 19, "int_neg": 20,
      "int_min": 21, "integer1": 22, "integer7": 23, "integer0": 24, "integer_min": 25, "date_time": 26, "time": 27, "date": 28,
      "duration": 29, "other": 30, "other2": 31, "str_en_gb": 32, "str_minus_nan": 33}
LEXICAL = {4: b"true", 5: b"true", 6: b"wahr", 7: b"", 32: b"colour", 33: b"-nan"}     # the strings' lexical forms (rdfgpu_store_set_strings)


def split_i128(v):
    u = v & ((1 << 128) - 1)
    lo, hi = u & ((1 << 64) - 1), u >> 64
    return (lo - (1 << 64) if lo >= 1 << 63 else lo, hi - (1 << 64) if hi >= 1 << 63 else hi)


def typed_table():
    """(rdfgpu_typed_value rows, the i128 side table) of TABLE."""
    tv = np.zeros(N_IDS, TV_DTYPE)
    decs = []
    for i, (tag, p) in enumerate(TABLE):
        lo, aux, flags = 0, 0, 0
        if tag in (abi.TV_NAMED_NODE, abi.TV_BLANK_NODE, abi.TV_DURATION, abi.TV_INT, abi.TV_INTEGER, abi.TV_FLOAT):
            lo = p
        elif tag == abi.TV_DOUBLE:
            lo = p - (1 << 64) if p >= 1 << 63 else p
        elif tag == abi.TV_BOOLEAN:
            lo = int(p)
        elif tag == abi.TV_STRING:
            lo, aux, flags = p[0], p[1], abi.TVF_EMPTY_STRING if p[2] else 0
        elif tag == abi.TV_DECIMAL:
            lo = len(decs); decs.append(p)
        elif tag in TIMESTAMPS:
            lo, aux = len(decs), int(p[1]); decs.append(p[0])
        elif tag == abi.TV_OTHER:
            lo, aux = p
        tv[i] = (lo, aux, tag, flags, 0)
    dec = np.array([split_i128(d) for d in decs], np.int64).reshape(len(decs), 2)
    return tv, dec


def string_heap():
    """(offsets, heap) for rdfgpu_store_set_strings: the lexical forms of LEXICAL, nothing for the other ids."""
    off = np.zeros(N_IDS + 1, np.uint64)
    heap = bytearray()
    for i in range(N_IDS):
        off[i] = len(heap)
        heap += LEXICAL.get(i, b"")
    off[N_IDS] = len(heap)
    return off, bytes(heap)


def enc(i):
    """ENC_TV: id 0 and ids beyond the table are the null value"""
    return TABLE[i] if 0 < i < N_IDS else NULL


# ---------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------
def sparql_if(test, a, b):
    if test[0] != abi.TV_BOOLEAN:          # Boolean::try_from: only an xsd:boolean converts — not the EBV
        return NULL
    return a if test[1] else b


def coalesce_tv(*vs):
    for v in vs:
        if v[0] != abi.TV_NULL:
            return v
    return NULL


def coalesce_id(*ids):
    for i in ids:
        if i != 0:
            return i
    return 0


def tv_bool(b):
    return (abi.TV_BOOLEAN, bool(b))


def is_iri(v):
    return NULL if v[0] == abi.TV_NULL else tv_bool(v[0] == abi.TV_NAMED_NODE)


def is_blank(v):
    return NULL if v[0] == abi.TV_NULL else tv_bool(v[0] == abi.TV_BLANK_NODE)


def is_literal(v):
    return NULL if v[0] == abi.TV_NULL else tv_bool(v[0] not in (abi.TV_NAMED_NODE, abi.TV_BLANK_NODE))


def is_numeric(v):
    return NULL if v[0] == abi.TV_NULL else tv_bool(v[0] in NUMERIC)


def _as_f64(v):
    tag, p = v
    if tag == abi.TV_DOUBLE:
        return f64_of(p)
    if tag == abi.TV_FLOAT:
        return np.float64(f32_of(p))
    if tag == abi.TV_DECIMAL:
        return np.float64(p) / np.float64(E18)          # exact for this table's decimals
    return np.float64(p)


def _as_f32(v):
    tag, p = v
    return f32_of(p) if tag == abi.TV_FLOAT else np.float32(_as_f64(v))


def tv_equal(a, b):
    """`=`: True / False / None (incomparable: an error)"""
    ta, tb = a[0], b[0]
    if ta == abi.TV_NULL or tb == abi.TV_NULL:
        return None
    nodes = (abi.TV_NAMED_NODE, abi.TV_BLANK_NODE)
    if ta in nodes or tb in nodes:           # IRIs and blank nodes order before / among each other: comparable with everything
        return ta == tb and a[1] == b[1]
    if ta == abi.TV_STRING:
        if tb != abi.TV_STRING or a[1][1] != b[1][1]:
            return None
        return a[1][0] == b[1][0]
    if ta == abi.TV_BOOLEAN:
        return a[1] == b[1] if tb == abi.TV_BOOLEAN else None
    if ta in NUMERIC:
        if tb not in NUMERIC:
            return None
        if abi.TV_DOUBLE in (ta, tb):
            x, y = _as_f64(a), _as_f64(b)
        elif abi.TV_FLOAT in (ta, tb):
            x, y = _as_f32(a), _as_f32(b)
        elif abi.TV_DECIMAL in (ta, tb):
            return (a[1] if ta == abi.TV_DECIMAL else a[1] * E18) == (b[1] if tb == abi.TV_DECIMAL else b[1] * E18)
        else:
            return a[1] == b[1]
        if np.isnan(x) or np.isnan(y):
            return None
        return bool(x == y)
    if ta == abi.TV_OTHER:
        return True if (tb == abi.TV_OTHER and a[1] == b[1]) else None
    if ta in TIMESTAMPS:
        if tb != ta:
            return None
        (x, tx), (y, ty) = a[1], b[1]
        if tx == ty:
            return x == y
        shift = 50400 * E18                   # the value without a timezone may lie 14 h either way
        cmp_ = lambda p, q: (p > q) - (p < q)
        plus, minus = (cmp_(x, y + shift), cmp_(x, y - shift)) if tx else (cmp_(x + shift, y), cmp_(x - shift, y))
        return plus == 0 if plus == minus else None
    return None                               # durations


def ebv(v):
    """0 / 1 / 2 (error)"""
    tag, p = v
    if tag == abi.TV_BOOLEAN:
        return int(p)
    if tag in (abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL):
        return int(p != 0)
    if tag == abi.TV_FLOAT:
        return int(f32_of(p) != 0)            # NaN != 0
    if tag == abi.TV_DOUBLE:
        return int(f64_of(p) != 0)
    if tag == abi.TV_STRING:
        return 2 if p[1] != 0 else int(not p[2])
    return 2


def and3(a, b):
    return 0 if a == 0 or b == 0 else 2 if a == 2 or b == 2 else 1


def or3(a, b):
    return 1 if a == 1 or b == 1 else 2 if a == 2 or b == 2 else 0


def not3(a):
    return 2 if a == 2 else 1 - a


def bool_as_term(b):
    return NULL if b == 2 else tv_bool(b)


def sparql_in(lhs, members):
    """rewrite_in: the OR chain of EBV(lhs = e), false for the empty list, as a term"""
    chain = None
    for e in members:
        eq = tv_equal(lhs, e)
        t = 2 if eq is None else int(eq)      # EBV of a boolean / of the error value
        chain = t if chain is None else or3(chain, t)
    return bool_as_term(0 if chain is None else chain)


def sparql_not_in(lhs, members):
    return bool_as_term(not3(ebv(sparql_in(lhs, members))))


def lang_equals(v, tag):
    """LANG(v) = "tag": a literal without a language has the tag "", IRIs / blank nodes / null are errors"""
    if v[0] in (abi.TV_NULL, abi.TV_NAMED_NODE, abi.TV_BLANK_NODE):
        return NULL
    return tv_bool(LANGUAGE_TAGS[v[1][1] if v[0] == abi.TV_STRING else 0] == tag)


def tv_abs(v):
    """ABS (numeric.rs:20-28), for the nested case: checked for int / integer / decimal, the sign bit cleared for float / double"""
    tag, p = v
    if tag == abi.TV_INT:
        return NULL if p == -2 ** 31 else (tag, abs(p))
    if tag == abi.TV_INTEGER:
        return NULL if p == -2 ** 63 else (tag, abs(p))
    if tag == abi.TV_DECIMAL:
        return NULL if p == -2 ** 127 else (tag, abs(p))
    if tag == abi.TV_FLOAT:
        return (tag, p & 0x7FFFFFFF)
    if tag == abi.TV_DOUBLE:
        return (tag, p & 0x7FFFFFFFFFFFFFFF)
    return NULL


def record(v):
    """a typed value as the (tag, lo, hi) of an rdfgpu_agg_value (numeric, boolean or the error value: what a value column carries)"""
    tag, p = v
    if tag == abi.TV_NULL:
        return (0, 0, 0)
    if tag == abi.TV_BOOLEAN:
        return (tag, int(p), 0)
    if tag == abi.TV_DECIMAL:
        lo, hi = split_i128(p)
        return (tag, lo, hi)
    if tag == abi.TV_DOUBLE:
        return (tag, p - (1 << 64) if p >= 1 << 63 else p, 0)
    assert tag in (abi.TV_INT, abi.TV_INTEGER, abi.TV_FLOAT), tag
    return (tag, p, 0)


# ---------------------------------------------------------------------------------------------------
# expressions that carry their own reference: X.expr is the plan's program, X.fn(row) what the reference says of a row of object ids
# ---------------------------------------------------------------------------------------------------
class X:
    def __init__(self, expr, fn):
        self.expr, self.fn = expr, fn


def literal(v):
    """a typed literal of the plan for the value v (numeric, boolean, IRI or simple / tagged string by rank)"""
    tag, p = v
    if tag == abi.TV_NULL:
        return P.lit_tv(tag)                  # the error value as a constant
    if tag == abi.TV_STRING:
        return P.lit_tv(tag, p[0], aux=p[1], flags=abi.TVF_EMPTY_STRING if p[2] else 0)
    if tag == abi.TV_DECIMAL:
        return P.decimal(p)
    if tag == abi.TV_DOUBLE:
        return P.lit_tv(tag, p - (1 << 64) if p >= 1 << 63 else p)
    if tag == abi.TV_BOOLEAN:
        return P.boolean(p)
    return P.lit_tv(tag, p)


def xcol(c): return X(P.col(c), lambda r: r[c])
def xenc(c): return X(P.ENC_TV(P.col(c)), lambda r: enc(r[c]))
def xlit(v): return X(literal(v), lambda r: v)
def xif(t, a, b): return X(P.IF(t.expr, a.expr, b.expr), lambda r: sparql_if(t.fn(r), a.fn(r), b.fn(r)))
def xcoalesce(*es): return X(P.COALESCE(*[e.expr for e in es]), lambda r: coalesce_tv(*[e.fn(r) for e in es]))
def xcoalesce_id(*es): return X(P.COALESCE(*[e.expr for e in es]), lambda r: coalesce_id(*[e.fn(r) for e in es]))
def xenc_of(e): return X(P.ENC_TV(e.expr), lambda r: enc(e.fn(r)))
def xis_iri(e): return X(P.IS_IRI(e.expr), lambda r: is_iri(e.fn(r)))
def xis_blank(e): return X(P.IS_BLANK(e.expr), lambda r: is_blank(e.fn(r)))
def xis_literal(e): return X(P.IS_LITERAL(e.expr), lambda r: is_literal(e.fn(r)))
def xis_numeric(e): return X(P.IS_NUMERIC(e.expr), lambda r: is_numeric(e.fn(r)))
def xin(lhs, es): return X(P.IN(lhs.expr, [e.expr for e in es]), lambda r: sparql_in(lhs.fn(r), [e.fn(r) for e in es]))
def xnot_in(lhs, es): return X(P.NOT_IN(lhs.expr, [e.expr for e in es]), lambda r: sparql_not_in(lhs.fn(r), [e.fn(r) for e in es]))
def xlang_equals(e, tag): return X(P.LANG_EQUALS(e.expr, tag, LANGUAGE_TAGS), lambda r: lang_equals(e.fn(r), tag))
def xabs(e): return X(P.ABS(e.expr), lambda r: tv_abs(e.fn(r)))
def xebv(e): return X(P.EBV(e.expr), lambda r: ebv(e.fn(r)))
def xnot(e): return X(P.NOT(e.expr), lambda r: not3(e.fn(r)))
def xor(a, b): return X(P.OR(a.expr, b.expr), lambda r: or3(a.fn(r), b.fn(r)))
def xand(a, b): return X(P.AND(a.expr, b.expr), lambda r: and3(a.fn(r), b.fn(r)))
def xbool_as_term(e): return X(P.BOOLEAN_AS_TERM(e.expr), lambda r: bool_as_term(e.fn(r)))
def xbound(e): return X(P.BOUND(e.expr), lambda r: int(e.fn(r) != 0))


IN_MEMBERS = [TABLE[ID["integer7"]], TABLE[ID["f64"]], TABLE[ID["str_en"]], TABLE[ID["iri2"]], TABLE[ID["true"]]]


def boolean_forms(a=0, b=1, c=2):
    """name -> X of kind TV(boolean | null) over the id columns a, b, c: every op alone, and nested"""
    A, B, C_ = xenc(a), xenc(b), xenc(c)
    nested = xif(xis_numeric(A), xabs(A), xcoalesce(B, xlit((abi.TV_INTEGER, 0))))      # IF(IS_NUMERIC(x), ABS(x), COALESCE(y, 0))
    return {
        "is_iri": xis_iri(A), "is_blank": xis_blank(A), "is_literal": xis_literal(A), "is_numeric": xis_numeric(A),
        "in_0": xin(A, []), "in_1": xin(A, [xlit(IN_MEMBERS[0])]), "in_5": xin(A, [xlit(m) for m in IN_MEMBERS]),
        "in_column": xin(A, [B, xlit(IN_MEMBERS[1])]),
        "not_in": xnot_in(A, [xlit(m) for m in IN_MEMBERS[:3]]),
        "if": xis_literal(xif(A, B, C_)),                       # the test is ANY typed value: only the two booleans choose
        "if_ebv": xis_iri(xif(xbool_as_term(xebv(A)), B, C_)),  # .. and the EBV form a plan writes when it wants that
        "coalesce": xis_numeric(xcoalesce(A, B, C_)),
        "coalesce_1": xis_blank(xcoalesce(A)),
        "coalesce_id": xis_literal(xenc_of(xcoalesce_id(xcol(a), xcol(b)))),
        "nested": xis_numeric(nested),
        "nested_in": xin(nested, [xlit((abi.TV_INT, 5)), xlit((abi.TV_DOUBLE, f64_bits(7.0)))]),      # (IN repeats its left side per member: 40 nodes a program)
    }


def value_forms(a=0, b=1, c=2):
    """name -> X whose value is numeric, boolean or the error value on every row: what a computed column or an aggregate can carry"""
    A, B = xenc(a), xenc(b)
    number = lambda e: xif(xis_numeric(e), e, xlit(NULL))      # e where it is numeric, else the error value
    out = dict(boolean_forms(a, b, c))
    out["nested_value"] = xif(xis_numeric(A), xabs(A), xcoalesce(number(B), xlit((abi.TV_INTEGER, 0))))
    out["if_value"] = xif(xis_literal(A), xlit((abi.TV_INT, 3)), xlit((abi.TV_DECIMAL, 5 * E18 // 10)))
    out["coalesce_value"] = xcoalesce(number(A), number(B), xlit((abi.TV_DOUBLE, f64_bits(-1.0))))
    return out


def filter_forms(a=0, b=1, c=2):
    """.. and what only a predicate may hold (LANGMATCHES-style tables are refused in computed columns and aggregate inputs)"""
    out = dict(boolean_forms(a, b, c))
    for tag in ("", "en", "en-GB", "fr"):
        out[f"lang_equals_{tag or 'none'}"] = xlang_equals(xenc(a), tag)
    return out


def id_columns(n, n_cols=3):
    """n rows of object ids that walk the table — id 0 and ids beyond it included — with different strides, and a row number column"""
    k = np.arange(n, dtype=np.int64)      # (periods without a common factor: the columns' combinations do not repeat within the largest table)
    cols = [((k * s + o) % (N_IDS + d)).astype(np.uint32) for s, o, d in ((1, 0, 9), (5, 3, 7), (11, 7, 13))[:n_cols]]
    return cols + [(k + 1).astype(np.uint32)]


ROW_COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 4097]     # one lane, the wave edge, the workgroup-tile edge, a second sweep

# ---------------------------------------------------------------------------------------------------
# hand-written truth tables, over ids of TABLE (0 = the error value)
# ---------------------------------------------------------------------------------------------------
_T, _F, _N, _ONE, _S, _I = ID["true"], ID["false"], 0, ID["integer1"], ID["str"], ID["iri"]     # the string's lexical form is "true"
_V, _W = ID["integer7"], ID["f64"]
IF_TRUTH = [   # (test, then, else, expected)
    (_T, _V, _W, _V), (_T, _V, _N, _V), (_T, _N, _W, _N), (_T, _N, _N, _N),
    (_F, _V, _W, _W), (_F, _V, _N, _N), (_F, _N, _W, _W), (_F, _N, _N, _N),
    (_N, _V, _W, _N), (_N, _V, _N, _N), (_N, _N, _W, _N), (_N, _N, _N, _N),
    (_ONE, _V, _W, _N), (_ONE, _V, _N, _N), (_ONE, _N, _W, _N), (_ONE, _N, _N, _N),        # the integer 1 is no boolean: not the EBV
    (_S, _V, _W, _N), (_S, _V, _N, _N), (_S, _N, _W, _N), (_S, _N, _N, _N),                # nor is the string "true"
    (_I, _V, _W, _N), (_I, _V, _N, _N), (_I, _N, _W, _N), (_I, _N, _N, _N),
]
_C = [ID["integer7"], ID["f64"], ID["str_en"], ID["iri"], ID["false"], ID["dec"], ID["blank"], ID["date_time"]]    # eight distinct values
COALESCE_TRUTH = [   # (operands, expected): every position of the first non-error among 1, 2, 3 and 8 operands, and all errors
    ([_C[0]], _C[0]), ([0], 0),
    ([_C[0], _C[1]], _C[0]), ([0, _C[1]], _C[1]), ([0, 0], 0),
    ([_C[0], _C[1], _C[2]], _C[0]), ([0, _C[1], _C[2]], _C[1]), ([0, 0, _C[2]], _C[2]), ([0, 0, 0], 0), ([_C[0], 0, _C[2]], _C[0]),
    (_C[:], _C[0]), ([0] + _C[1:], _C[1]), ([0, 0] + _C[2:], _C[2]), ([0, 0, 0] + _C[3:], _C[3]), ([0, 0, 0, 0] + _C[4:], _C[4]),
    ([0, 0, 0, 0, 0] + _C[5:], _C[5]), ([0] * 6 + _C[6:], _C[6]), ([0] * 7 + _C[7:], _C[7]), ([0] * 8, 0), ([0, _C[1], 0, _C[3], 0, 0, 0, _C[7]], _C[1]),
]
COALESCE_ID_TRUTH = [([4], 4), ([0], 0), ([0, 3], 3), ([5, 3], 5), ([0, 0, 9], 9), ([0, 0, 0], 0), ([0, BEYOND, 2], BEYOND), ([0] * 7 + [1], 1), ([0] * 8, 0)]


# ---------------------------------------------------------------------------------------------------
# the LeftMark join: a dict and a loop
# ---------------------------------------------------------------------------------------------------
def mark_join(L, R, on, flt=None):
    """[(left row index, mark)] in left order.  L, R: lists of columns; on: [(left col, right col)]; flt(left row, right row) -> bool:
    the join filter is exactly true.  Null keys equal nothing."""
    nl, nr = (len(L[0]) if L else 0), (len(R[0]) if R else 0)
    lrows = list(zip(*[c.tolist() for c in L])) if nl else []
    rrows = list(zip(*[c.tolist() for c in R])) if nr else []
    table = {}
    for r in rrows:
        key = tuple(r[b] for _, b in on)
        if 0 not in key:
            table.setdefault(key, []).append(r)
    out = []
    for j, l in enumerate(lrows):
        key = tuple(l[a] for a, _ in on)
        cands = [] if 0 in key else table.get(key, [])
        out.append((j, any(flt is None or flt(l, r) for r in cands)))
    return out


def rand_cols(rng, n, ncols, n_ids, null_frac=0.1):
    cols = [rng.integers(1, n_ids, n).astype(np.uint32) for _ in range(ncols)]
    for c in cols:
        c[rng.random(n) < null_frac] = 0
    return cols


def mark_filters(n_left_cols):
    """name -> (Expr over [left cols, right cols], the same as a Python function of (left row, right row)); columns 1 / 2 of the left,
    1 of the right"""
    w = n_left_cols
    vm = xand(xor(xebv(xis_numeric(xenc(2))), xebv(xin(xenc(w + 1), [xenc(1), xlit(TABLE[ID["integer7"]])]))), xbound(xcol(1)))
    return {
        "none": (None, None),
        "id_pair": (P.ID_NEQ(P.col(1), P.col(w + 1)), lambda l, r: l[1] != 0 and r[1] != 0 and l[1] != r[1]),
        "vm": (vm.expr, lambda l, r: vm.fn(tuple(l) + tuple(r)) == 1),
    }


def tv_equal_term(a, b):
    eq = tv_equal(a, b)
    return NULL if eq is None else tv_bool(eq)


def xeq(a, b): return X(P.EQ(a.expr, b.expr), lambda r: tv_equal_term(a.fn(r), b.fn(r)))
def xid_eq(a, b): return X(P.ID_EQ(a.expr, b.expr), lambda r: 2 if a.fn(r) == 0 or b.fn(r) == 0 else int(a.fn(r) == b.fn(r)))
