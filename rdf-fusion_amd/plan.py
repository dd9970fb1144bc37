"""Host-side plan description, named after the reference's types.

This is the Python mirror of what the Rust host hands over the C ABI: scan instructions
(`MemIndexScanInstruction`, lib/storage/src/memory/storage/scan_instructions.rs:247-318),
expression programs (the `PhysicalExpr` trees of FilterExec / JoinFilter built from the UDFs in
lib/extensions/src/functions/builtin.rs:101-186) and the operator tree
(DataSourceExec / FilterExec / HashJoinExec / CrossJoinExec / NestedLoopJoinExec as printed in
bench/tests/plans/snapshots/*Q5 (Execution Plan).snap).  It only builds ``rdfgpu_plan_desc``
structs; it computes nothing.
"""
import ctypes as C
import struct

from . import abi


# ----------------------------------------------------------------------------------------------
# scan instructions
# ----------------------------------------------------------------------------------------------
class MemIndexScanPredicate:
    """scan_instructions.rs:157-166"""

    def __init__(self, kind, ids=None, lo=0, hi=0, var=None):
        self.kind, self.ids, self.lo, self.hi, self.var = kind, ids, lo, hi, var

    @staticmethod
    def false():
        return MemIndexScanPredicate(abi.PRED_FALSE)

    @staticmethod
    def in_(ids):
        return MemIndexScanPredicate(abi.PRED_IN, ids=sorted(set(int(i) for i in ids)))

    @staticmethod
    def between(lo, hi):
        return MemIndexScanPredicate(abi.PRED_BETWEEN, lo=int(lo), hi=int(hi))

    @staticmethod
    def equal_to(var):
        return MemIndexScanPredicate(abi.PRED_EQUAL_TO, var=var)

    def __repr__(self):  # Display impl scan_instructions.rs:213-237
        if self.kind == abi.PRED_FALSE:
            return "false"
        if self.kind == abi.PRED_IN:
            return f"== {self.ids[0]}" if len(self.ids) == 1 else "in (" + ", ".join(map(str, self.ids)) + ")"
        if self.kind == abi.PRED_BETWEEN:
            return f"in ({self.lo}..{self.hi})"
        return f"== {self.var}"


class MemIndexScanInstruction:
    """scan_instructions.rs:247-318"""

    def __init__(self, kind, var=None, predicate=None):
        self.kind, self.var, self.predicate = kind, var, predicate

    @staticmethod
    def traverse(object_id=None):
        """`traverse(1)` in the reference tests = Traverse(Some(In{1}))."""
        if object_id is None:
            return MemIndexScanInstruction(abi.TRAVERSE)
        return MemIndexScanInstruction(abi.TRAVERSE, predicate=MemIndexScanPredicate.in_([object_id]))

    @staticmethod
    def traverse_with_predicate(predicate):
        return MemIndexScanInstruction(abi.TRAVERSE, predicate=predicate)

    @staticmethod
    def scan(var):
        return MemIndexScanInstruction(abi.SCAN, var=var)

    @staticmethod
    def scan_with_predicate(var, predicate):
        return MemIndexScanInstruction(abi.SCAN, var=var, predicate=predicate)


def quad_pattern(subject, predicate, obj, graph="default", graph_variable=None):
    """MemQuadStorageSnapshot::plan_pattern_evaluation (snapshot.rs:84-131): int = constant object
    id, str = variable.  `graph`: "default" | "all" | "named" | list of graph ids
    (MemIndexScanInstruction::from_active_graph, scan_instructions.rs:323-355)."""
    P, I = MemIndexScanPredicate, MemIndexScanInstruction
    if graph == "default":
        gp = P.in_([0])
    elif graph == "all":
        gp = None
    elif graph == "named":
        gp = P.between(1, 0xFFFFFFFF)
    else:
        gp = P.in_(list(graph))
    g = I(abi.SCAN, var=graph_variable, predicate=gp) if graph_variable else I(abi.TRAVERSE, predicate=gp)

    def term(t):
        return I.scan(t) if isinstance(t, str) else I.traverse(int(t))

    return [g, term(subject), term(predicate), term(obj)]


# ----------------------------------------------------------------------------------------------
# expressions (postfix programs)
# ----------------------------------------------------------------------------------------------
class Expr:
    def __init__(self, nodes):
        self.nodes = nodes  # list of (op, tag, flags, u, lo, hi)

    def _bin(self, other, op):
        return Expr(self.nodes + other.nodes + [(op, 0, 0, 0, 0, 0)])

    def _un(self, op):
        return Expr(self.nodes + [(op, 0, 0, 0, 0, 0)])


def col(i):
    return Expr([(abi.EX_COLUMN, 0, 0, int(i), 0, 0)])


def lit_id(object_id):
    return Expr([(abi.EX_LIT_ID, 0, 0, int(object_id), 0, 0)])


def lit_tv(tag, lo=0, aux=0, flags=0, hi=0):
    return Expr([(abi.EX_LIT_TV, int(tag), int(flags), int(aux), int(lo), int(hi))])


def lit_bool(v):
    return Expr([(abi.EX_LIT_BOOL, 0, 0, 2 if v is None else int(bool(v)), 0, 0)])


def integer(v):          # plan text "9:120"
    return lit_tv(abi.TV_INTEGER, int(v))


def int32(v):
    return lit_tv(abi.TV_INT, int(v))


def boolean(v):
    return lit_tv(abi.TV_BOOLEAN, int(bool(v)))


def double(v):
    return lit_tv(abi.TV_DOUBLE, struct.unpack("<q", struct.pack("<d", float(v)))[0])


def float32(v):
    return lit_tv(abi.TV_FLOAT, struct.unpack("<I", struct.pack("<f", float(v)))[0])


def decimal(scaled_i128):
    """scaled_i128 = value * 10**18 (decimal.rs:9-21)."""
    v = int(scaled_i128) & ((1 << 128) - 1)
    lo, hi = v & ((1 << 64) - 1), v >> 64
    to_i64 = lambda x: x - (1 << 64) if x >= (1 << 63) else x
    return lit_tv(abi.TV_DECIMAL, to_i64(lo), hi=to_i64(hi))


def _timestamp(tag, scaled_i128, has_timezone, tz_minutes=0):
    v = int(scaled_i128) & ((1 << 128) - 1)
    lo, hi = v & ((1 << 64) - 1), v >> 64
    to_i64 = lambda x: x - (1 << 64) if x >= (1 << 63) else x
    if tz_minutes and not has_timezone:
        raise ValueError("a timestamp without a timezone has no offset")
    if not -840 <= int(tz_minutes) <= 840:
        raise ValueError("a timezone offset lies within -14:00 .. +14:00")
    # `u`: bit 0 = has a timezone, bits 16..31 = the offset in minutes as int16 (read by the date parts only)
    return lit_tv(tag, to_i64(lo), aux=(1 if has_timezone else 0) | ((int(tz_minutes) & 0xFFFF) << 16), hi=to_i64(hi))


def date_time(scaled_i128, has_timezone, tz_minutes=0):
    """xsd:dateTime literal: Timestamp value * 10**18 (rdf_fusion_amd.xsd.parse_date_time) + timezone presence + the offset in minutes
    (what YEAR .. MINUTES shift the UTC instant by; comparisons never look at it)."""
    return _timestamp(abi.TV_DATE_TIME, scaled_i128, has_timezone, tz_minutes)


def date(scaled_i128, has_timezone):
    return _timestamp(abi.TV_DATE, scaled_i128, has_timezone)


def time(scaled_i128, has_timezone):
    return _timestamp(abi.TV_TIME, scaled_i128, has_timezone)


def ENC_TV(e): return e._un(abi.EX_ENC_TV)
def GT(a, b): return a._bin(b, abi.EX_GT)
def LT(a, b): return a._bin(b, abi.EX_LT)
def GEQ(a, b): return a._bin(b, abi.EX_GEQ)
def LEQ(a, b): return a._bin(b, abi.EX_LEQ)
def EQ(a, b): return a._bin(b, abi.EX_EQ)
def NEQ(a, b): return a._bin(b, abi.EX_NEQ)
def ADD(a, b): return a._bin(b, abi.EX_ADD)
def SUB(a, b): return a._bin(b, abi.EX_SUB)
def EBV(e): return e._un(abi.EX_EBV)


# Numeric expressions (include/rdfgpu.h, ABI 4 addendum): scalar/numeric/{mul,div,unary_minus,unary_plus,abs,round,ceil,floor}.rs and the
# XSD constructor functions scalar/conversion/cast_*.rs.
def MUL(a, b): return a._bin(b, abi.EX_MUL)
def DIV(a, b): return a._bin(b, abi.EX_DIV)
def NEG(e): return e._un(abi.EX_NEG)
def PLUS(e): return e._un(abi.EX_PLUS)
def ABS(e): return e._un(abi.EX_ABS)
def ROUND(e): return e._un(abi.EX_ROUND)
def CEIL(e): return e._un(abi.EX_CEIL)
def FLOOR(e): return e._un(abi.EX_FLOOR)


# The parts of an xsd:dateTime (include/rdfgpu.h, ABI 4 addendum): scalar/dates_and_times/{year,month,day,hours,minutes,seconds}.rs.  Only a
# dateTime yields a value (xsd:integer; SECONDS: xsd:decimal), every other kind is the error value.
def YEAR(e): return e._un(abi.EX_YEAR)
def MONTH(e): return e._un(abi.EX_MONTH)
def DAY(e): return e._un(abi.EX_DAY)
def HOURS(e): return e._un(abi.EX_HOURS)
def MINUTES(e): return e._un(abi.EX_MINUTES)
def SECONDS(e): return e._un(abi.EX_SECONDS)


def CAST(e, tag):
    """xsd:<type>(e): `tag` = abi.TV_BOOLEAN / TV_INT / TV_INTEGER / TV_DECIMAL / TV_FLOAT / TV_DOUBLE (another tag is the library's to refuse)."""
    return Expr(e.nodes + [(abi.EX_CAST, 0, 0, int(tag), 0, 0)])


def CAST_LEX(e, tag):
    """xsd:<type>(e) that also PARSES a simple literal (RDFGPU_EX_CAST_LEX; the reference's FromStr impls: f32::from_str, Decimal::from_str,
    ..): on every other operand exactly CAST.  `tag` as for CAST."""
    return Expr(e.nodes + [(abi.EX_CAST_LEX, 0, 0, int(tag), 0, 0)])


def xsd_string(e):
    """xsd:string(ENC_TV(col(c))) (scalar/conversion/cast_string.rs), lowered to RDFGPU_EX_CAST_STRING over the column's object id: ENC_TV
    keeps the id for strings only, and the cast needs the lexical form of IRIs and other literals (`"12.5"^^bsbm:USD`) too.  Anything but
    ENC_TV of a column has no id to take the lexical form from: refused here."""
    n = e.nodes
    if len(n) != 2 or n[0][0] != abi.EX_COLUMN or n[1][0] != abi.EX_ENC_TV:
        raise ValueError("xsd_string takes ENC_TV(col(c)): the cast reads the lexical form through the column's object id")
    return Expr([n[0], (abi.EX_CAST_STRING, 0, 0, 0, 0, 0)])


def _cast(e, tag, lexical): return CAST_LEX(e, tag) if lexical else CAST(e, tag)
# lexical=True: the operand may be a simple literal (xsd:float(xsd:string(ENC_TV(price)))), parsed on the device (CAST_LEX)
def xsd_boolean(e, lexical=False): return _cast(e, abi.TV_BOOLEAN, lexical)
def xsd_int(e, lexical=False): return _cast(e, abi.TV_INT, lexical)
def xsd_integer(e, lexical=False): return _cast(e, abi.TV_INTEGER, lexical)
def xsd_decimal(e, lexical=False): return _cast(e, abi.TV_DECIMAL, lexical)
def xsd_float(e, lexical=False): return _cast(e, abi.TV_FLOAT, lexical)
def xsd_double(e, lexical=False): return _cast(e, abi.TV_DOUBLE, lexical)


def REGEX(e, pattern, flags=""):
    """REGEX(value, "pattern"[, "flags"]) with constant pattern / flags (scalar/strings/regex.rs:47-141)."""
    enc = lambda x: x.encode("utf-8") if isinstance(x, str) else bytes(x)
    return Expr(e.nodes + [(abi.EX_REGEX, 0, 0, (enc(pattern), enc(flags), abi.EX_REGEX), 0, 0)])


def REGEX_VAR(e, pattern_expr, patterns, flags=""):
    """REGEX(value, ?pattern[, "flags"]) with a per-row pattern (regex.rs:59-76): `pattern_expr` = ENC_TV of the pattern column,
    `patterns` = {object id: pattern text} of every distinct pattern literal that can occur (the host's dictionary knows them)."""
    enc = lambda x: x.encode("utf-8") if isinstance(x, str) else bytes(x)
    table = tuple((int(pid), enc(txt)) for pid, txt in sorted(patterns.items()))
    return Expr(e.nodes + pattern_expr.nodes + [(abi.EX_REGEX_VAR, 0, 0, ("var", table, enc(flags)), 0, 0)])


def _string_fn(op):
    def f(e, needle, language_id=0):
        """<fn>(value, "constant"[@lang]) — contains.rs / str_starts.rs / str_ends.rs; language_id = the constant's
        language id in the typed-value table's `aux` numbering (0 = simple literal)."""
        b = needle.encode("utf-8") if isinstance(needle, str) else bytes(needle)
        return Expr(e.nodes + [(op, 0, 0, (b, b"", op), int(language_id), 0)])
    return f


CONTAINS, STRSTARTS, STRENDS = _string_fn(abi.EX_CONTAINS), _string_fn(abi.EX_STRSTARTS), _string_fn(abi.EX_STRENDS)


# String-valued expressions (include/rdfgpu.h, ABI 3).  STR takes the column itself (an object id): over an object-id column
# the reference evaluates STR in the plain-term encoding, i.e. on the lexical form as written (scalar/terms/str.rs:42).
def STR(e):
    return e._un(abi.EX_STR)


def lit_str(text, language_id=0):
    """A string constant with its bytes (what a computed string is compared with); language_id as in the typed-value table."""
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    return Expr([(abi.EX_LIT_STR, 0, 0, (b, b"", abi.EX_LIT_STR), int(language_id), 0)])


def STRLEN(e):
    return e._un(abi.EX_STRLEN)


def SUBSTR(e, start, length=None):
    """SUBSTR(str, start[, length]) — scalar/strings/sub_str.rs; start / length are expressions (e.g. integer(2))."""
    nodes = e.nodes + start.nodes + (length.nodes if length is not None else [])
    return Expr(nodes + [(abi.EX_SUBSTR, 0, 0, 3 if length is not None else 2, 0, 0)])


def UCASE(e):
    return e._un(abi.EX_UCASE)


def LCASE(e):
    return e._un(abi.EX_LCASE)


def STRBEFORE(a, b):
    """STRBEFORE(a, b) — scalar/strings/str_before.rs: the part of a before b's first occurrence (a's language), "" if there is none."""
    return Expr(a.nodes + b.nodes + [(abi.EX_STRBEFORE, 0, 0, 0, 0, 0)])


def STRAFTER(a, b):
    """STRAFTER(a, b) — scalar/strings/str_after.rs."""
    return Expr(a.nodes + b.nodes + [(abi.EX_STRAFTER, 0, 0, 0, 0, 0)])


def lang_matches(language_tag, language_range):
    """LANGMATCHES on two plain strings, as scalar/strings/lang_matches.rs:52-69 evaluates it: "*" matches every
    non-empty tag; otherwise the subtags ('-' separated) are zipped with the longer side padded: a range subtag that is
    missing from, or differs (ASCII case-insensitively) from, the tag's subtag at that position is a mismatch."""
    if language_range == "*":
        return language_tag != ""
    r, l = language_range.split("-"), language_tag.split("-")
    ascii_lower = lambda x: "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in x)
    for i in range(max(len(r), len(l))):
        if i < len(r) and (i >= len(l) or ascii_lower(r[i]) != ascii_lower(l[i])):
            return False
    return True


def LANGMATCHES_LANG(e, language_range, language_tags):
    """LANGMATCHES(LANG(value), "range") — BSBM explore Q8's FILTER.  `language_tags[i]` = the tag of language id i in the
    typed-value table's `aux` numbering (language_tags[0] must be "": literals without a language).  The host resolves
    the range against that (small) dictionary; the device reads one verdict byte per language id."""
    if not language_tags or language_tags[0] != "":
        raise ValueError("language_tags[0] is the empty tag")
    verdicts = bytes(1 if lang_matches(t, language_range) else 0 for t in language_tags)
    return Expr(e.nodes + [(abi.EX_LANG_IN, 0, 0, (verdicts, b"", abi.EX_LANG_IN), 0, 0)])


def LANG_EQUALS(e, tag, language_tags):
    """LANG(value) = "tag" — scalar/terms/lang.rs:49-55 under `=`: the same op as LANGMATCHES_LANG with a table that is 1 exactly for the
    language ids whose tag IS `tag` (byte for byte: `=` on simple literals).  A literal without a language has the tag "" (id 0); IRIs,
    blank nodes and the null value are the error value.  `language_tags` as for LANGMATCHES_LANG."""
    if not language_tags or language_tags[0] != "":
        raise ValueError("language_tags[0] is the empty tag")
    verdicts = bytes(1 if t == tag else 0 for t in language_tags)
    return Expr(e.nodes + [(abi.EX_LANG_IN, 0, 0, (verdicts, b"", abi.EX_LANG_IN), 0, 0)])


# Functional forms and term tests (include/rdfgpu.h, ABI 4 addendum).  Every operand is evaluated for every row, as in the reference.
def IF(test, a, b):
    """IF(test, a, b) — scalar/functional_form/sparql_if.rs: `test` is a typed value that must be an xsd:boolean (Boolean::try_from, not the
    EBV: write BOOLEAN_AS_TERM(EBV(x)) for that); anything else is the error value.  The chosen branch comes out unchanged."""
    return Expr(test.nodes + a.nodes + b.nodes + [(abi.EX_IF, 0, 0, 0, 0, 0)])


def COALESCE(*es):
    """COALESCE(e1, ..) — DataFusion's `coalesce` (lib/functions/src/registry.rs:264-270): the first operand that is not the error value
    (typed values) or not 0 (object ids); 1 to abi.MAX_STACK operands, all typed values or all object ids."""
    if not 1 <= len(es) <= abi.MAX_STACK:
        raise ValueError(f"COALESCE takes 1 to {abi.MAX_STACK} operands")
    return Expr([n for e in es for n in e.nodes] + [(abi.EX_COALESCE, 0, 0, len(es), 0, 0)])


def IS_IRI(e): return e._un(abi.EX_IS_IRI)
def IS_BLANK(e): return e._un(abi.EX_IS_BLANK)
def IS_LITERAL(e): return e._un(abi.EX_IS_LITERAL)
def IS_NUMERIC(e): return e._un(abi.EX_IS_NUMERIC)


def IN(lhs, es):
    """lhs IN (e1, ..) — expression_rewriter.rs:302-322 (rewrite_in): BOOLEAN_AS_TERM of the OR chain of EBV(EQ(lhs, e_i)), left to right;
    the empty list is BOOLEAN_AS_TERM(false).  A typed value (boolean, or the error value where no member is equal and one comparison
    is an error)."""
    chain = None
    for e in es:
        t = EBV(EQ(lhs, e))
        chain = t if chain is None else OR(chain, t)
    return BOOLEAN_AS_TERM(lit_bool(False) if chain is None else chain)


def NOT_IN(lhs, es):
    """lhs NOT IN (e1, ..): BOOLEAN_AS_TERM(NOT(EBV(IN(lhs, es))))."""
    return BOOLEAN_AS_TERM(NOT(EBV(IN(lhs, es))))


def ID_EQ(a, b): return a._bin(b, abi.EX_ID_EQ)
def ID_NEQ(a, b): return a._bin(b, abi.EX_ID_NEQ)
def AND(a, b): return a._bin(b, abi.EX_AND)
def OR(a, b): return a._bin(b, abi.EX_OR)
def NOT(e): return e._un(abi.EX_NOT)
def IS_COMPATIBLE(a, b): return a._bin(b, abi.EX_IS_COMPATIBLE)
def BOUND(e): return e._un(abi.EX_BOUND)
def BOOLEAN_AS_TERM(e): return e._un(abi.EX_BOOL_AS_TV)


# ----------------------------------------------------------------------------------------------
# operator tree
# ----------------------------------------------------------------------------------------------
class PlanDescription:
    """Owns the ctypes arrays behind one ``rdfgpu_plan_desc``."""

    def __init__(self, nodes, exprs, pool, root, n_columns, regexes=(), flags=0, value_columns=()):
        self.n_columns = n_columns  # output width per node (host-side bookkeeping)
        self.flags = int(flags)     # abi.PLAN_*
        self.value_columns = list(value_columns)   # abi.PLAN_AGG_COLUMNS: which output columns of the root are aggregate value columns
        self._nodes = (abi.PlanNode * max(1, len(nodes)))(*nodes)
        self._exprs = (abi.ExprNode * max(1, len(exprs)))(*exprs)
        self._pool = (C.c_uint32 * max(1, len(pool)))(*pool)
        self._regex_bytes = [(bytes(r[0]), bytes(r[1]), int(r[2]) if len(r) > 2 else 0) for r in regexes]      # keeps the char buffers alive
        self._regexes = (abi.Regex * max(1, len(regexes)))(*[abi.Regex(p, f, len(p), len(f), pid, 0) for p, f, pid in self._regex_bytes])
        self.desc = abi.PlanDesc(self._nodes, len(nodes), root, self._exprs, len(exprs), self._pool,
                                 len(pool), self.flags, self._regexes, len(regexes), 0)
        self.root = root

    @property
    def width(self):
        return self.n_columns[self.root]


class PlanBuilder:
    def __init__(self):
        self.nodes, self.exprs, self.pool, self.width = [], [], [], []
        self.names = []          # per node: the names of its output columns (variables), for plan display
        self.patterns = []       # per node: the quad pattern of a DataSourceExec (four MemIndexScanInstructions) or None
        self.regexes = []
        self._regex_keys = []
        self.vars = {}
        self.values = []         # per node: which of its output columns are aggregate value columns (build(agg_columns=True))

    # -- helpers -------------------------------------------------------------------------------
    def _var(self, name):
        return self.vars.setdefault(name, len(self.vars))

    def _instr(self, ins):
        out = abi.ScanInstruction()
        out.kind = ins.kind
        out.var = self._var(ins.var) if ins.kind == abi.SCAN else 0
        p = ins.predicate
        if p is None:
            out.pred = abi.PRED_NONE
        elif p.kind == abi.PRED_IN:
            out.pred, out.a, out.b = abi.PRED_IN, len(self.pool), len(p.ids)
            self.pool.extend(p.ids)
        elif p.kind == abi.PRED_BETWEEN:
            out.pred, out.a, out.b = abi.PRED_BETWEEN, p.lo, p.hi
        elif p.kind == abi.PRED_EQUAL_TO:
            out.pred, out.a = abi.PRED_EQUAL_TO, self._var(p.var)
        else:
            out.pred = abi.PRED_FALSE
        return out

    def _expr(self, node, e):
        if e is None:
            node.expr_off, node.expr_len = 0, 0
            return
        node.expr_off, node.expr_len = len(self.exprs), len(e.nodes)
        for (op, tag, flags, u, lo, hi) in e.nodes:
            if op == abi.EX_REGEX_VAR:
                # one regex entry per announced pattern, contiguous: u = first entry, lo = count
                _, table, fl = u
                u, lo = len(self.regexes), len(table)
                for pid, txt in table:
                    self._regex_keys.append(("var", pid, txt, fl))
                    self.regexes.append((txt, fl, pid))
            elif op in (abi.EX_REGEX, abi.EX_CONTAINS, abi.EX_STRSTARTS, abi.EX_STRENDS, abi.EX_LANG_IN, abi.EX_LIT_STR):
                # u carries (pattern, flags, op): register the plan constant (one entry per function), keep its index
                if u not in self._regex_keys:
                    self._regex_keys.append(u)
                    self.regexes.append(u[:2])
                u = self._regex_keys.index(u)
            self.exprs.append(abi.ExprNode(op, tag, flags, 0, u, lo, hi))

    def _proj(self, node, projection, full):
        if projection is None:
            node.proj_off, node.n_proj = 0, abi.NO_PROJECTION
            return full
        node.proj_off, node.n_proj = len(self.pool), len(projection)
        self.pool.extend(int(c) for c in projection)
        return len(projection)

    def _push(self, node, width, names=None, pattern=None):
        self.nodes.append(node)
        self.width.append(width)
        self.names.append(list(names) if names is not None else [f"c{i}" for i in range(width)])
        self.patterns.append(pattern)
        self.values.append(self._value_columns(node, width))
        assert len(self.names[-1]) == width
        return len(self.nodes) - 1

    def _value_columns(self, node, width):
        """Which output columns of `node` carry aggregate values when they are columns: an AggregateExec's aggregates, and whatever a
        projection, filter, sort or join hands on of its inputs' (a semi / anti join: of its left input's)."""
        if node.kind == abi.NODE_AGGREGATE:     # a key that is a value column stays one (build(value_keys=True)); the aggregates always are
            below = self.values[node.left]
            n_keys = width - node.table_cols       # (keys beyond the bound have no slot: the library refuses the node)
            keys = [_agg_key_col(node, k) if k < abi.MAX_GROUP_KEYS else len(below) for k in range(n_keys)]
            return [bool(c < len(below) and below[c]) for c in keys] + [True] * node.table_cols
        if node.kind in (abi.NODE_DATA_SOURCE, abi.NODE_TABLE) or node.left < 0:
            return [False] * width
        if node.kind == abi.NODE_EXTEND:        # the kept columns as the input has them, then the computed ones
            full = list(self.values[node.left])
            kept = range(len(full)) if node.n_proj == abi.NO_PROJECTION else [self.pool[node.proj_off + q] for q in range(node.n_proj)]
            return [full[c] for c in kept] + [True] * node.table_cols
        full = list(self.values[node.left])
        binary = node.kind in (abi.NODE_HASH_JOIN, abi.NODE_CROSS_JOIN, abi.NODE_NESTED_LOOP_JOIN)
        if binary and node.join_type == abi.JOIN_LEFT_MARK and node.kind != abi.NODE_CROSS_JOIN:
            full += [True]                      # [left cols, mark]: the mark is a value column of the join's own
        elif binary and node.join_type not in (abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI):
            full += self.values[node.right]
        if node.n_proj == abi.NO_PROJECTION:
            return full[:width] + [False] * (width - len(full))
        return [full[self.pool[node.proj_off + q]] if self.pool[node.proj_off + q] < len(full) else False for q in range(node.n_proj)]

    def _projected(self, full_names, projection):
        return list(full_names) if projection is None else [full_names[int(c)] for c in projection]

    # -- operators -----------------------------------------------------------------------------
    def data_source(self, instructions):
        """DataSourceExec(MemQuadPatternDataSource): four instructions in G,S,P,O order."""
        n = abi.PlanNode(kind=abi.NODE_DATA_SOURCE, left=-1, right=-1)
        seen, width = [], 0
        for i, ins in enumerate(instructions):
            n.scan[i] = self._instr(ins)
            if ins.kind == abi.SCAN and ins.var not in seen:
                seen.append(ins.var)
                width += 1
        n.n_proj = abi.NO_PROJECTION
        return self._push(n, width, seen, list(instructions))

    def filter(self, child, predicate, projection=None):
        n = abi.PlanNode(kind=abi.NODE_FILTER, left=child, right=-1)
        self._expr(n, predicate)
        return self._push(n, self._proj(n, projection, self.width[child]), self._projected(self.names[child], projection))

    def projection(self, child, columns, names=None):
        """ProjectionExec of plain columns; `names` renames them (`count(..)@1 as monthCount`: display only)."""
        n = abi.PlanNode(kind=abi.NODE_PROJECTION, left=child, right=-1)
        return self._push(n, self._proj(n, columns, self.width[child]), self._projected(self.names[child], columns) if names is None else names)

    def _join_output(self, left, right, join_type):
        """Columns a join outputs before its projection: [left, right], the left ones only for LeftSemi / LeftAnti, or the left ones and
        the mark for LeftMark."""
        if join_type in (abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI):
            return self.width[left], self.names[left]
        if join_type == abi.JOIN_LEFT_MARK:
            return self.width[left] + 1, self.names[left] + ["mark"]
        return self.width[left] + self.width[right], self.names[left] + self.names[right]

    def hash_join(self, left, right, on, join_type=abi.JOIN_INNER, filter=None, projection=None):
        """HashJoinExec(CollectLeft).  join_type LEFT_SEMI / LEFT_ANTI: the output is the left columns (the projection indexes
        them); the filter still sees [left cols, right cols]."""
        n = abi.PlanNode(kind=abi.NODE_HASH_JOIN, left=left, right=right, join_type=join_type)
        n.n_keys = len(on)
        for k, (l, r) in enumerate(on):
            n.left_keys[k], n.right_keys[k] = l, r
        self._expr(n, filter)
        width, names = self._join_output(left, right, join_type)
        return self._push(n, self._proj(n, projection, width), self._projected(names, projection))

    def cross_join(self, left, right):
        n = abi.PlanNode(kind=abi.NODE_CROSS_JOIN, left=left, right=right, join_type=abi.JOIN_INNER)
        n.n_proj = abi.NO_PROJECTION
        return self._push(n, self.width[left] + self.width[right], self.names[left] + self.names[right])

    def nested_loop_join(self, left, right, join_type=abi.JOIN_INNER, filter=None, projection=None):
        n = abi.PlanNode(kind=abi.NODE_NESTED_LOOP_JOIN, left=left, right=right, join_type=join_type)
        self._expr(n, filter)
        width, names = self._join_output(left, right, join_type)
        return self._push(n, self._proj(n, projection, width), self._projected(names, projection))

    def table(self, slot, n_cols, names=None):
        n = abi.PlanNode(kind=abi.NODE_TABLE, left=-1, right=-1, table_slot=slot, table_cols=n_cols)
        n.n_proj = abi.NO_PROJECTION
        return self._push(n, n_cols, names)

    def topk(self, left, keys, limit, group=None, projection=None, tie_break=True):
        """DISTINCT + ORDER BY keys ASC LIMIT `limit` (per `group` column if given) — the AggregateExec(first_value) +
        SortExec TopK(fetch) pair above the path in the reference's explore plans.  keys = [(column, abi.SORT_BY_ID |
        abi.SORT_BY_TERM | abi.SORT_BY_DOUBLE), ...].  The AggregateExec groups by the sort expressions AND the raw output
        columns, so (`tie_break`) every output column that is not yet a key by id is appended as one: at most 4 keys."""
        keys = [(int(c), int(how)) for c, how in keys]
        out_cols = list(range(self.width[left])) if projection is None else [int(c) for c in projection]
        if tie_break:
            for c in out_cols:
                if (group is None or c != int(group)) and (c, abi.SORT_BY_ID) not in keys:
                    keys.append((c, abi.SORT_BY_ID))
        if len(keys) > 4:
            raise ValueError("TopK: more than 4 sort keys (ORDER BY keys + output columns)")
        n = abi.PlanNode(kind=abi.NODE_TOPK, left=left, right=-1, n_keys=len(keys), table_cols=int(limit),
                         table_slot=0 if group is None else int(group) + 1)
        for i, (c, how) in enumerate(keys):
            n.left_keys[i], n.right_keys[i] = c, how
        return self._push(n, self._proj(n, projection, self.width[left]), self._projected(self.names[left], projection))

    def sort(self, child, keys, fetch=None, projection=None):
        """SortExec (abi.NODE_SORT): ORDER BY `keys` = [(column, how, descending), ...] (1 to 4), `how` = abi.SORT_BY_ID / SORT_BY_TERM /
        SORT_BY_DOUBLE over an object-id column or abi.SORT_BY_VALUE over a value column; `fetch` keeps the first rows only
        (`SortExec: TopK(fetch=10)`; None: all).  No DISTINCT; rows equal on every key keep their input order.  A value column stays a
        value column of the output."""
        keys = [(int(c), int(how), bool(desc)) for c, how, desc in keys]
        n = abi.PlanNode(kind=abi.NODE_SORT, left=child, right=-1, n_keys=len(keys), table_cols=0 if fetch is None else int(fetch))
        for i, (c, how, desc) in enumerate(keys[:abi.MAX_KEYS]):      # (more than MAX_KEYS is the library's to refuse)
            n.left_keys[i], n.right_keys[i] = c, how | (abi.SORT_DESC if desc else 0)
        return self._push(n, self._proj(n, projection, self.width[child]), self._projected(self.names[child], projection))

    def sparql_order_by(self, child, keys, limit=None):
        """ORDER BY .. [LIMIT limit] over `child`: keys = [(column, descending), ...] or [(column, descending, how), ...].  A value column
        (an aggregate, a computed column) sorts BY_VALUE; an object-id column by `how` (default abi.SORT_BY_ID)."""
        full = []
        for key in keys:
            c, desc = int(key[0]), bool(key[1])
            how = abi.SORT_BY_VALUE if self.values[child][c] else (int(key[2]) if len(key) > 2 else abi.SORT_BY_ID)
            full.append((c, how, desc))
        return self.sort(child, full, fetch=limit)

    def union(self, left, right, projection=None):
        """UnionExec: bag union of two inputs with the same columns (SPARQL UNION; Q4 (Execution Plan).snap:11)."""
        if self.width[left] != self.width[right]:
            raise ValueError("UNION inputs differ in width")
        n = abi.PlanNode(kind=abi.NODE_UNION, left=left, right=right)
        return self._push(n, self._proj(n, projection, self.width[left]), self._projected(self.names[left], projection))

    def closure(self, left, allow_cross_graph_paths=False):
        """KleenePlusClosureExec over inner paths (graph, start, end) — the `+` of a SPARQL property path."""
        if self.width[left] != 3:
            raise ValueError("inner paths are (graph, start, end)")
        n = abi.PlanNode(kind=abi.NODE_CLOSURE, left=left, right=-1, join_type=1 if allow_cross_graph_paths else 0)
        return self._push(n, self._proj(n, None, 3), self.names[left])

    def aggregate(self, left, group_by, aggregates=()):
        """AggregateExec(mode=Single): GROUP BY the columns `group_by` — 0 to 4 id columns; in a description built with value_keys=True up to
        8 columns, value columns (aggregates, computed columns) among them, grouped by the term their value stands for — with `aggregates` = [(abi.AGG_*, input column), ...]
        (at most 8; AGG_COUNT_STAR takes no column: None).  AGG_MIN / AGG_MAX need a description built with agg_columns=True; their answer
        is fixed and independent of row order (include/rdfgpu.h: an unbound row makes the group unbound, a value that is not numeric fails
        the execute).  The input of AGG_SUM / AGG_AVG / AGG_MIN / AGG_MAX may be an `Expr` over the input's columns that
        yields a typed value (`MUL(ENC_TV(col(1)), ENC_TV(col(2)))`): it goes into the pool as abi.AGG_INPUT_EXPR | offset of
        (expr_off, expr_len).  Output: the keys in order, then the aggregates, named like DataFusion's display (`COUNT(y)`,
        `SUM(MUL(ENC_TV(a), ENC_TV(b)))`).  Only the key columns are ids: a node with aggregates must be the plan's root — unless the
        description is built with agg_columns=True, where the aggregates are value columns that the operators above read (build, sparql_having)."""
        group_by = [int(c) for c in group_by]
        aggregates = [(int(fn), c if c is None or isinstance(c, Expr) else int(c)) for fn, c in aggregates]
        names = self.names[left]
        n = abi.PlanNode(kind=abi.NODE_AGGREGATE, left=left, right=-1, n_keys=len(group_by), table_cols=len(aggregates),
                         table_slot=len(self.pool))
        for k, c in enumerate(group_by[:abi.MAX_GROUP_KEYS]):      # keys 0..3 in left_keys[], 4..7 in right_keys[] (an aggregate has no other use for them)
            if k < abi.MAX_KEYS:
                n.left_keys[k] = c
            else:
                n.right_keys[k - abi.MAX_KEYS] = c
        n.n_keys = len(group_by)           # (more than the bound is the library's to refuse)
        first = len(self.pool) + 2 * len(aggregates)   # the (expr_off, expr_len) pairs follow the aggregate list
        n_expr = 0
        for fn, c in aggregates:
            if isinstance(c, Expr):
                self.pool.extend([fn, abi.AGG_INPUT_EXPR | (first + 2 * n_expr)])
                n_expr += 1
            else:
                self.pool.extend([fn, 0 if c is None else c])
        labels = []
        for fn, c in aggregates:
            if isinstance(c, Expr):
                holder = abi.PlanNode()
                self._expr(holder, c)
                self.pool.extend([holder.expr_off, holder.expr_len])
                labels.append(_agg_label(fn, format_expr(self.exprs[holder.expr_off:holder.expr_off + holder.expr_len], names, at=False)))
            else:
                labels.append(_agg_label(fn, None if c is None else names[c]))
        n.n_proj = abi.NO_PROJECTION
        out = [names[c] for c in group_by] + labels
        return self._push(n, len(out), out)

    def extend(self, child, exprs, keep=None, names=None):
        """ProjectionExec with expressions (SPARQL Extend; abi.NODE_EXTEND): the columns `keep` of `child` (None: all), then one computed
        column per `Expr` of `exprs` (1 to 8) — a program over ALL of the child's columns that leaves a typed value, e.g. BSBM Business
        Intelligence Q3's `DIV(xsd_float(ENC_TV(col(1))), ENC_TV(col(2)))`.  The computed columns are value columns (`value_columns`),
        named `names` (default: the expression as DataFusion prints it).  In the pool: k pairs (expr_off, expr_len) at table_slot.  The
        description must be built with agg_columns=True."""
        exprs = list(exprs)
        full = self.names[child]
        n = abi.PlanNode(kind=abi.NODE_EXTEND, left=child, right=-1, table_cols=len(exprs))
        kept = self._proj(n, None if keep is None else [int(c) for c in keep], self.width[child])
        pairs = []
        for e in exprs:
            holder = abi.PlanNode()
            self._expr(holder, e)
            pairs += [holder.expr_off, holder.expr_len]
        n.table_slot = len(self.pool)
        self.pool.extend(pairs)
        if names is None:
            names = [format_expr(self.exprs[pairs[2 * q]:pairs[2 * q] + pairs[2 * q + 1]], full, at=False) for q in range(len(exprs))]
        if len(names) != len(exprs):
            raise ValueError("extend: one name per expression")
        return self._push(n, kept + len(exprs), self._projected(full, keep) + list(names))

    def sparql_bind(self, child, expr, name):
        """BIND(expr AS ?name) / SELECT (expr AS ?name): every column of `child`, then the computed one."""
        return self.extend(child, [expr], keep=None, names=[name])

    def build(self, root, agg_columns=False, value_keys=False):
        """value_keys=True (only with agg_columns=True) sets abi.PLAN_VALUE_KEYS: an AggregateExec groups by up to 8 columns, value columns
        among them.  agg_columns=True sets abi.PLAN_AGG_COLUMNS: an AggregateExec with aggregates may sit anywhere, its output is the keys and then
        one value column per aggregate (n_columns counts them), and FilterExec / joins / further aggregates above read the values through
        ENC_TV.  Without it the description is what it always was: aggregates at the root only, values through GpuPlan.aggregate_values."""
        if value_keys and not agg_columns:
            raise ValueError("value_keys=True needs agg_columns=True: value columns exist only in such a plan")
        return PlanDescription(self.nodes, self.exprs, self.pool, root, list(self.width), list(self.regexes),
                               flags=(abi.PLAN_AGG_COLUMNS if agg_columns else 0) | (abi.PLAN_VALUE_KEYS if value_keys else 0),
                               value_columns=[c for c, v in enumerate(self.values[root]) if v] if agg_columns else [])

    def sparql_having(self, agg, predicate, projection=None):
        """HAVING over an AggregateExec (or anything that carries its value columns): a FilterExec whose predicate reads the aggregates'
        values through ENC_TV of their columns — BSBM Business Intelligence Q3 (Execution Plan).snap:17,
        `FilterExec: EBV(GT(INT64_AS_TERM(count@1), 9:0))`, and Q6 (Execution Plan).snap:6, `FilterExec: EBV(GT(avg@1, MUL(avg@2, 1.5)))`.
        INT64_AS_TERM(count) is the identity here: a COUNT's value already is an xsd:integer, so `ENC_TV(col(1))` stands for it.  The
        description must be built with agg_columns=True."""
        return self.filter(agg, predicate, projection)


    # -- SparqlJoinNode lowering ------------------------------------------------------------------
    def sparql_join(self, left, right, join_type=abi.JOIN_INNER, filter=None):
        """SparqlJoinLoweringRule (lib/logical/src/join/rewrite.rs:71-221) for inputs whose shared variables are
        non-nullable (object-id columns of quad patterns): no shared variable => CrossJoinExec (inner, :74-96) or a
        left join without keys and without a filter (what DataFusion plans as NestedLoopJoinExec, ..Q2 (Execution
        Plan).snap:6-8); otherwise an equi-join on ALL shared variables (:126-168, NullEqualsNothing :89) whose output
        is the left fields followed by the right fields not already present (join/logical.rs:251-279).  Nullable shared
        variables (IS_COMPATIBLE + COALESCE, :183-221, :327-345) are outside this path."""
        ln, rn = self.names[left], self.names[right]
        shared = [v for v in ln if v in rn]
        if not shared:
            if join_type == abi.JOIN_INNER:
                if filter is not None:
                    return self.nested_loop_join(left, right, abi.JOIN_INNER, filter=filter)
                return self.cross_join(left, right)
            return self.nested_loop_join(left, right, abi.JOIN_LEFT, filter=filter)
        on = [(ln.index(v), rn.index(v)) for v in shared]
        keep = list(range(len(ln))) + [len(ln) + i for i, v in enumerate(rn) if v not in ln]
        return self.hash_join(left, right, on, join_type=join_type, filter=filter, projection=keep)

    # -- EXISTS / NOT EXISTS / MINUS lowering -----------------------------------------------------
    def _semi_anti(self, left, right, anti, nullable, minus, mark=False):
        ln, rn = self.names[left], self.names[right]
        shared = sorted(v for v in ln if v in rn)
        jt = abi.JOIN_LEFT_MARK if mark else abi.JOIN_LEFT_ANTI if anti else abi.JOIN_LEFT_SEMI
        if not any(v in nullable for v in shared):
            on = [(ln.index(v), rn.index(v)) for v in shared]
            return self.hash_join(left, right, on, join_type=jt)
        w = len(ln)
        f = None
        for v in shared:
            c = IS_COMPATIBLE(col(ln.index(v)), col(w + rn.index(v)))
            f = c if f is None else AND(f, c)
        if minus:
            some = None
            for v in shared:
                b = AND(BOUND(col(ln.index(v))), BOUND(col(w + rn.index(v))))
                some = b if some is None else OR(some, b)
            f = AND(f, some)
        return self.nested_loop_join(left, right, jt, filter=f)

    def sparql_exists(self, outer, inner, negate=False, nullable=()):
        """FILTER EXISTS { inner } (negate: FILTER NOT EXISTS) over `outer`: the correlated subquery of
        lib/logical/src/expr_builder_context.rs:197-300, as DataFusion decorrelates it into a LeftSemi / LeftAnti join whose
        output is `outer`'s columns.  S = the variables `outer` and `inner` share:
          - S empty: the test is whether `inner` has any row at all — a NestedLoopJoinExec without a filter;
          - no variable of S nullable: a hash join on every variable of S, in sorted order (the correlation predicates
            `outer.v = inner.v`, :275-276, become the equi-keys);
          - some variable of S in `nullable`: IS_COMPATIBLE per shared variable, AND-ed, as the join filter of a
            NestedLoopJoinExec (no equi-keys are left)."""
        if not any(v in self.names[inner] for v in self.names[outer]):
            return self.nested_loop_join(outer, inner, abi.JOIN_LEFT_ANTI if negate else abi.JOIN_LEFT_SEMI)
        return self._semi_anti(outer, inner, negate, set(nullable), minus=False)

    def sparql_exists_value(self, outer, inner, nullable=()):
        """EXISTS { inner } as an OPERAND (`FILTER(?p > 10 || EXISTS {..})`, `BIND(IF(EXISTS {..}, ..))`): the same correlated subquery,
        which DataFusion decorrelates into a LeftMark join wherever EXISTS is not a conjunct of its own.  The lowering of sparql_exists —
        the same keys, the same IS_COMPATIBLE filter for nullable shared variables — with abi.JOIN_LEFT_MARK: `outer`'s columns, every
        row once and in order, followed by the mark, a boolean value column (`ENC_TV(col(mark))` reads it; NOT EXISTS is
        `NOT(EBV(ENC_TV(col(mark))))`).  The description must be built with agg_columns=True."""
        if not any(v in self.names[inner] for v in self.names[outer]):
            return self.nested_loop_join(outer, inner, abi.JOIN_LEFT_MARK)
        return self._semi_anti(outer, inner, False, set(nullable), minus=False, mark=True)

    def sparql_minus(self, left, right, nullable=()):
        """left MINUS right (lib/logical/src/minus/rewrite.rs:58-130): a LeftAnti join.  No shared variable: `left` unchanged
        (:62-64).  Shared variables all non-nullable: anti join on them.  Otherwise a NestedLoopJoinExec whose filter is the AND
        over S of IS_COMPATIBLE(l.v, r.v), AND-ed with the OR over S of BOUND(l.v) AND BOUND(r.v) (:93-135: a right row that binds
        none of the shared variables removes nothing)."""
        if not any(v in self.names[right] for v in self.names[left]):
            return left
        return self._semi_anti(left, right, True, set(nullable), minus=True)


# ----------------------------------------------------------------------------------------------
# plan display, in the reference's format (bench/tests/plans/snapshots/*.snap; DataSourceExec lines as
# MemQuadPatternDataSource::fmt_as prints them, pattern_data_source.rs:80-105)
# ----------------------------------------------------------------------------------------------
_BIN = {abi.EX_GT: "GT", abi.EX_LT: "LT", abi.EX_GEQ: "GEQ", abi.EX_LEQ: "LEQ", abi.EX_EQ: "EQ", abi.EX_ADD: "ADD", abi.EX_SUB: "SUB",
        abi.EX_IS_COMPATIBLE: "IS_COMPATIBLE", abi.EX_MUL: "MUL", abi.EX_DIV: "DIV"}
_JOIN_TYPE_NAMES = {abi.JOIN_INNER: "Inner", abi.JOIN_LEFT: "Left", abi.JOIN_LEFT_SEMI: "LeftSemi", abi.JOIN_LEFT_ANTI: "LeftAnti",
                    abi.JOIN_LEFT_MARK: "LeftMark"}
_UN = {abi.EX_ENC_TV: "ENC_TV", abi.EX_EBV: "EBV", abi.EX_BOUND: "BOUND", abi.EX_BOOL_AS_TV: "BOOLEAN_AS_TERM",
       abi.EX_NEG: "MINUS", abi.EX_PLUS: "PLUS", abi.EX_ABS: "ABS", abi.EX_ROUND: "ROUND", abi.EX_CEIL: "CEIL", abi.EX_FLOOR: "FLOOR",
       abi.EX_YEAR: "YEAR", abi.EX_MONTH: "MONTH", abi.EX_DAY: "DAY", abi.EX_HOURS: "HOURS", abi.EX_MINUTES: "MINUTES", abi.EX_SECONDS: "SECONDS",
       # BuiltinName's spelling (lib/extensions/src/functions/builtin.rs:144-147)
       abi.EX_IS_IRI: "isIRI", abi.EX_IS_BLANK: "isBLANK", abi.EX_IS_LITERAL: "isLITERAL", abi.EX_IS_NUMERIC: "isNUMERIC"}
# BuiltinName::CastBoolean .. CastDouble as the reference's plans print them (`xsd:integer(..)`)
_CAST = {abi.TV_BOOLEAN: "xsd:boolean", abi.TV_INT: "xsd:int", abi.TV_INTEGER: "xsd:integer", abi.TV_DECIMAL: "xsd:decimal",
         abi.TV_FLOAT: "xsd:float", abi.TV_DOUBLE: "xsd:double"}


def _agg_key_col(node, k):
    """group column k of an AggregateExec node: 0..3 in left_keys[], 4..7 in right_keys[]"""
    return node.left_keys[k] if k < abi.MAX_KEYS else node.right_keys[k - abi.MAX_KEYS]


def _agg_label(fn, column, at=None):
    """An aggregate as DataFusion names it: COUNT(*), COUNT(y), COUNT(DISTINCT y), SUM(y), AVG(y) (`y@1` with the column index)."""
    arg = "*" if column is None else (column if at is None else f"{column}@{at}")
    if fn == abi.AGG_COUNT_STAR:
        return "COUNT(*)"
    if fn in (abi.AGG_COUNT_DISTINCT, abi.AGG_SUM_DISTINCT, abi.AGG_AVG_DISTINCT):
        return f"{abi.AGG_NAMES[fn].split('(')[0]}(DISTINCT {arg})"
    return f"{abi.AGG_NAMES.get(fn, f'AGG{fn}')}({arg})"


def format_expr(nodes, names, at=True):
    """A postfix program as DataFusion prints the PhysicalExpr tree (`EBV(GT(ENC_TV(value1@1), 9:136))`,
    `product@0 != <object id>`, `.. AND ..`); object-id literals print as the snapshots mask them (<c>).  `at=False`: columns by
    name only, as in an output column's name (`SUM(MUL(ENC_TV(a), ENC_TV(b)))`)."""
    st = []
    for n in nodes:
        op, tag, u, lo = n.op, n.tag, n.u, n.lo
        if op == abi.EX_COLUMN:
            st.append(f"{names[u]}@{u}" if at else f"{names[u]}")
        elif op == abi.EX_LIT_ID:
            st.append("<c>")
        elif op == abi.EX_LIT_TV:
            st.append(f"{tag}:{lo}")
        elif op == abi.EX_LIT_BOOL:
            st.append({0: "false", 1: "true", 2: "NULL"}[u])
        elif op in _UN:
            st.append(f"{_UN[op]}({st.pop()})")
        elif op in (abi.EX_CAST, abi.EX_CAST_LEX):
            st.append(f"{_CAST.get(u, f'cast{u}')}({st.pop()})")
        elif op == abi.EX_CAST_STRING:      # the id form of xsd:string(ENC_TV(c)), printed as the reference prints it
            st.append(f"xsd:string(ENC_TV({st.pop()}))")
        elif op in _BIN:
            b, a = st.pop(), st.pop()
            st.append(f"{_BIN[op]}({a}, {b})")
        elif op in (abi.EX_ID_EQ, abi.EX_ID_NEQ, abi.EX_AND, abi.EX_OR):
            b, a = st.pop(), st.pop()
            st.append(f"{a} {({abi.EX_ID_EQ: '=', abi.EX_ID_NEQ: '!=', abi.EX_AND: 'AND', abi.EX_OR: 'OR'})[op]} {b}")
        elif op == abi.EX_NOT:
            st.append(f"NOT {st.pop()}")
        elif op == abi.EX_IF:
            c, b, a = st.pop(), st.pop(), st.pop()
            st.append(f"IF({a}, {b}, {c})")
        elif op == abi.EX_COALESCE:
            args = [st.pop() for _ in range(u)][::-1]
            st.append(f"COALESCE({', '.join(args)})")
        else:
            st.append(f"op{op}({st.pop()})")
    assert len(st) == 1
    return st[0]


def explain(pb, root, choose_index=None, agg_columns=False):
    """The operator tree under `root`, one line per operator, indented like DataFusion's `displayable(plan).indent()`.
    `choose_index(instructions) -> abi.GSPO | GPOS | GOSP` names the index of a DataSourceExec (the library's
    rdfgpu_choose_index; default: engine.choose_index).  `agg_columns=True` (the plan as build(root, agg_columns=True) describes it): an
    AggregateExec line ends in `values=[COUNT(*)@1, ..]`, its aggregates as the value columns the operators above read."""
    if choose_index is None:
        from .engine import choose_index as _ci
        choose_index = lambda ins: _ci([PlanBuilder()._instr(i) for i in ins])
    lines = []

    def proj(i, full):
        n = pb.nodes[i]
        if n.n_proj == abi.NO_PROJECTION:
            return ""
        cols = [pb.pool[n.proj_off + q] for q in range(n.n_proj)]
        return ", projection=[" + ", ".join(f"{full[c]}@{c}" for c in cols) + "]"

    def term(ins):
        if ins.kind == abi.SCAN:
            return "?" + ins.var
        return "<c>"

    def walk(i, depth):
        n = pb.nodes[i]
        pad = "  " * depth
        if n.kind == abi.NODE_DATA_SOURCE:
            g, s_, p_, o_ = pb.patterns[i]
            idx = abi.INDEX_NAMES[choose_index(pb.patterns[i])]
            graph = f"graph=?{g.var}, " if g.kind == abi.SCAN else ""
            lines.append(f"{pad}DataSourceExec: [{idx}] {graph}subject={term(s_)}, predicate={term(p_)}, object={term(o_)}")
            return
        if n.kind == abi.NODE_FILTER:
            full = pb.names[n.left]
            e = format_expr(pb.exprs[n.expr_off:n.expr_off + n.expr_len], full)
            lines.append(f"{pad}FilterExec: {e}{proj(i, full)}")
            walk(n.left, depth + 1)
            return
        if n.kind in (abi.NODE_HASH_JOIN, abi.NODE_NESTED_LOOP_JOIN):
            ln, rn = pb.names[n.left], pb.names[n.right]
            jt = _JOIN_TYPE_NAMES[n.join_type]
            head = "HashJoinExec: mode=CollectLeft" if n.kind == abi.NODE_HASH_JOIN else "NestedLoopJoinExec:"
            sep = ", " if n.kind == abi.NODE_HASH_JOIN else " "
            text = f"{head}{sep}join_type={jt}"
            if n.kind == abi.NODE_HASH_JOIN:
                text += ", on=[" + ", ".join(f"({ln[n.left_keys[k]]}@{n.left_keys[k]}, {rn[n.right_keys[k]]}@{n.right_keys[k]})" for k in range(n.n_keys)) + "]"
            if n.expr_len:
                # DataFusion prints a JoinFilter over ITS OWN intermediate schema: only the referenced columns, numbered in
                # order of first use, left side first (`simProperty2@1 .. origProperty2@0`)
                ex = pb.exprs[n.expr_off:n.expr_off + n.expr_len]
                used = sorted({e.u for e in ex if e.op == abi.EX_COLUMN})
                renum = {c: k for k, c in enumerate(used)}
                both = ln + rn
                fake = [abi.ExprNode(e.op, e.tag, e.flags, 0, renum[e.u] if e.op == abi.EX_COLUMN else e.u, e.lo, e.hi) for e in ex]
                text += ", filter=" + format_expr(fake, [both[c] for c in used])
            out = ln if n.join_type in (abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI) else ln + ["mark"] if n.join_type == abi.JOIN_LEFT_MARK else ln + rn
            lines.append(f"{pad}{text}{proj(i, out)}")
            walk(n.left, depth + 1); walk(n.right, depth + 1)
            return
        if n.kind == abi.NODE_CROSS_JOIN:
            lines.append(f"{pad}CrossJoinExec")
            walk(n.left, depth + 1); walk(n.right, depth + 1)
            return
        if n.kind == abi.NODE_TABLE:
            lines.append(f"{pad}BoundTableExec: slot={n.table_slot}, columns=[{', '.join(pb.names[i])}]")
            return
        if n.kind == abi.NODE_AGGREGATE:
            full = pb.names[n.left]
            # a value key prints as the reference groups by it: the plain term of the value, `ENC_PT(year@7) as year`
            keys = [_agg_key_col(n, k) for k in range(min(n.n_keys, abi.MAX_GROUP_KEYS))]
            is_value = lambda c: c < len(pb.values[n.left]) and pb.values[n.left][c]
            gby = ", ".join((f"ENC_PT({full[c]}@{c}) as {full[c]}" if is_value(c) else f"{full[c]}@{c} as {full[c]}") for c in keys)
            aggs = []
            for a in range(n.table_cols):
                fn, c = pb.pool[n.table_slot + 2 * a], pb.pool[n.table_slot + 2 * a + 1]
                if fn != abi.AGG_COUNT_STAR and c & abi.AGG_INPUT_EXPR:
                    off, ln = pb.pool[c & ~abi.AGG_INPUT_EXPR], pb.pool[(c & ~abi.AGG_INPUT_EXPR) + 1]
                    aggs.append(_agg_label(fn, format_expr(pb.exprs[off:off + ln], full)))
                    continue
                aggs.append(_agg_label(fn, None if fn == abi.AGG_COUNT_STAR else full[c], c))
            values = ""
            if agg_columns and n.table_cols:   # the aggregates' values as output columns, `name@index`
                values = ", values=[" + ", ".join(f"{pb.names[i][n.n_keys + a]}@{n.n_keys + a}" for a in range(n.table_cols)) + "]"
            lines.append(f"{pad}AggregateExec: mode=Single, gby=[{gby}], aggr=[{', '.join(aggs)}]{values}")
            walk(n.left, depth + 1)
            return
        if n.kind == abi.NODE_EXTEND:       # `ProjectionExec: expr=[product@0 as product, .., DIV(..) as ratio]`
            full = pb.names[n.left]
            kept = range(len(full)) if n.n_proj == abi.NO_PROJECTION else [pb.pool[n.proj_off + q] for q in range(n.n_proj)]
            items = [f"{full[c]}@{c} as {full[c]}" for c in kept]
            for q in range(n.table_cols):
                off, ln = pb.pool[n.table_slot + 2 * q], pb.pool[n.table_slot + 2 * q + 1]
                ex = pb.exprs[off:off + ln]
                # ENC_TV of a value column is the identity (its value is a typed value already): the reference prints the column
                ex = [e for j, e in enumerate(ex) if not (e.op == abi.EX_ENC_TV and j and ex[j - 1].op == abi.EX_COLUMN
                                                          and ex[j - 1].u < len(full) and pb.values[n.left][ex[j - 1].u])]
                items.append(f"{format_expr(ex, full)} as {pb.names[i][len(kept) + q]}")
            lines.append(f"{pad}ProjectionExec: expr=[{', '.join(items)}]")
            walk(n.left, depth + 1)
            return
        if n.kind == abi.NODE_SORT:         # `SortExec: TopK(fetch=10), expr=[ratio@3 DESC, product@0 ASC]`
            full = pb.names[n.left]
            keys = ", ".join(f"{full[n.left_keys[k]]}@{n.left_keys[k]} {'DESC' if n.right_keys[k] & abi.SORT_DESC else 'ASC'}" for k in range(min(n.n_keys, abi.MAX_KEYS)))
            lines.append(f"{pad}SortExec: {f'TopK(fetch={n.table_cols}), ' if n.table_cols else ''}expr=[{keys}]{proj(i, full)}")
            walk(n.left, depth + 1)
            return
        name = {abi.NODE_PROJECTION: "ProjectionExec", abi.NODE_TOPK: "SortExec: TopK", abi.NODE_UNION: "UnionExec",
                abi.NODE_CLOSURE: "KleenePlusClosureExec"}[n.kind]
        lines.append(f"{pad}{name}")
        walk(n.left, depth + 1)
        if n.kind == abi.NODE_UNION:
            walk(n.right, depth + 1)

    walk(root, 0)
    return lines


def explain_logical_join(pb, node):
    """The LOGICAL form of a join node produced by PlanBuilder.sparql_join, as DataFusion prints it in the reference's
    join-lowering tests (lib/logical/src/join/rewrite.rs:411-437: `Cross Join: ` / `Left Join: `)."""
    n = pb.nodes[node]
    if n.kind == abi.NODE_CROSS_JOIN:
        return "Cross Join: "
    jt = "Inner" if n.join_type == abi.JOIN_INNER else "Left"
    on = ", ".join(f"{pb.names[n.left][n.left_keys[k]]} = {pb.names[n.right][n.right_keys[k]]}" for k in range(n.n_keys)) if n.kind == abi.NODE_HASH_JOIN else ""
    return f"{jt} Join: {on}"
