"""What rdfgpu_plan_compile refuses, and which refusal comes first (plan_compile.cpp).  Every case builds the smallest valid
PlanDescription over bound-table inputs (no data is loaded), breaks one field of it in place (where PlanBuilder itself would
refuse) and checks the status and a distinguishing part of the message.  The ordering cases carry two defects and check which
one is reported: nodes are checked in index order, a node's checks in their order, the string table before any node."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from rdf_fusion_amd.plan import PlanBuilder, col, AND, EBV, ENC_TV, REGEX, CONTAINS, STRSTARTS, STRLEN

INVALID, UNSUPPORTED = abi.ERR_INVALID, abi.ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def store(torch_cuda):
    return rf.GpuQuadStore()


@pytest.fixture(scope="module")
def store_with_strings(torch_cuda):
    gs = rf.GpuQuadStore()
    gs.set_strings(np.array([0, 0, 1], dtype=np.uint64), b"a")
    return gs


# ---- the smallest valid plans: (builder, root) ----------------------------------------------------------------------------
def hash_join():
    pb = PlanBuilder()
    return pb, pb.hash_join(pb.table(0, 2), pb.table(1, 2), on=[(0, 0)])          # nodes: table, table, join


def cross_join():
    pb = PlanBuilder()
    return pb, pb.cross_join(pb.table(0, 2), pb.table(1, 2))


def closure():
    pb = PlanBuilder()
    return pb, pb.closure(pb.table(0, 3))                                          # nodes: table, closure


def union():
    pb = PlanBuilder()
    return pb, pb.union(pb.table(0, 2), pb.table(1, 2))


def table():
    pb = PlanBuilder()
    return pb, pb.table(0, 2)


def topk():
    pb = PlanBuilder()
    return pb, pb.topk(pb.table(0, 2), [(0, abi.SORT_BY_ID)], 5)                   # keys: (0, by id), (1, by id) (the tie break)


def aggregate(fn=abi.AGG_COUNT, arg=1):
    pb = PlanBuilder()
    return pb, pb.aggregate(pb.table(0, 2), [0], [(fn, arg)])                      # pool: [fn, input(, expr_off, expr_len)]


def aggregate_below_a_table():
    pb, agg = aggregate()
    return pb, pb.table(1, 1)                                                       # the root is the node after the aggregate


def aggregate_with_a_consumer():
    pb, agg = aggregate()
    pb.projection(agg, [0])                                                         # checked, though the root (the aggregate) does not reach it
    return pb, agg


def projection():
    pb = PlanBuilder()
    return pb, pb.projection(pb.table(0, 2), [0])                                   # pool: [0]


def contains_filter():
    pb = PlanBuilder()
    return pb, pb.filter(pb.table(0, 2), EBV(CONTAINS(ENC_TV(col(0)), "x")))       # exprs: COLUMN, ENC_TV, CONTAINS, EBV


def two_string_functions():
    pb = PlanBuilder()
    both = AND(EBV(CONTAINS(ENC_TV(col(0)), "x")), EBV(STRSTARTS(ENC_TV(col(0)), "y")))   # exprs 2 and 6 are the functions
    return pb, pb.filter(pb.table(0, 2), both)


def strlen_filter():
    pb = PlanBuilder()
    return pb, pb.filter(pb.table(0, 2), EBV(STRLEN(ENC_TV(col(0)))))


def long_regex():
    pb = PlanBuilder()
    return pb, pb.filter(pb.table(0, 2), EBV(REGEX(ENC_TV(col(0)), "a" * 65)))


def node(i, **fields):
    def f(d):
        for k, v in fields.items():
            if isinstance(v, tuple):            # (index, value) of an array field
                getattr(d._nodes[i], k)[v[0]] = v[1]
            else:
                setattr(d._nodes[i], k, v)
    return f


def pool(i, v):
    def f(d):
        d._pool[i] = v
    return f


def expr(i, **fields):
    def f(d):
        for k, v in fields.items():
            setattr(d._exprs[i], k, v)
    return f


def both(*fs):
    def f(d):
        for g in fs:
            g(d)
    return f


def nothing(d):
    pass


CASES = [
    # hash join
    ("join: no key", hash_join, node(2, n_keys=0), INVALID, "node 2: HashJoinExec needs 1..4 keys"),
    ("join: five keys", hash_join, node(2, n_keys=5), INVALID, "node 2: HashJoinExec needs 1..4 keys"),
    ("join: left key out of range", hash_join, node(2, left_keys=(0, 2)), INVALID, "node 2: join key out of range"),
    ("join: right key out of range", hash_join, node(2, right_keys=(0, 7)), INVALID, "node 2: join key out of range"),
    ("join: type", hash_join, node(2, join_type=9), UNSUPPORTED, "node 2: join type 9"),
    ("cross join: filter", cross_join, node(2, expr_len=1), INVALID, "node 2: CrossJoinExec takes no filter / join type"),
    ("cross join: left", cross_join, node(2, join_type=abi.JOIN_LEFT), INVALID, "node 2: CrossJoinExec takes no filter / join type"),
    # closure, union, table
    ("closure: width", closure, node(0, table_cols=2), INVALID, "node 1: KleenePlusClosureExec input has 2 columns"),
    ("closure: flag", closure, node(1, join_type=2), INVALID, "node 1: allow_cross_graph_paths is 0 or 1"),
    ("union: widths", union, node(1, table_cols=3), INVALID, "node 2: UnionExec inputs have 2 and 3 columns"),
    ("table: columns", table, node(0, table_cols=17), UNSUPPORTED, "node 0: table with 17 columns"),
    # TopK
    ("topk: no key", topk, node(1, n_keys=0), UNSUPPORTED, "node 1: TopK with 0 sort keys (1 to 4)"),
    ("topk: five keys", topk, node(1, n_keys=5), UNSUPPORTED, "node 1: TopK with 5 sort keys (1 to 4)"),
    ("topk: fetch 0", topk, node(1, table_cols=0), UNSUPPORTED, "node 1: TopK fetch = 0"),
    ("topk: fetch 1025", topk, node(1, table_cols=1025), UNSUPPORTED, "node 1: TopK fetch = 1025"),
    ("topk: key column", topk, node(1, left_keys=(0, 9)), INVALID, "node 1: sort key column 9 out of range"),
    ("topk: sort mode", topk, node(1, right_keys=(0, 3)), INVALID, "node 1: unknown sort mode 3"),
    ("topk: group column", topk, node(1, table_slot=4), INVALID, "node 1: group column out of range"),
    ("topk: uncovered output", topk, node(1, right_keys=(1, abi.SORT_BY_TERM)), UNSUPPORTED, "node 1: TopK output column 1 is neither the group nor a sort key by id"),
    # aggregate
    ("aggregate: five group columns", aggregate, node(1, n_keys=5), UNSUPPORTED, "node 1: AggregateExec with 5 group columns (at most 4)"),
    ("aggregate: nine aggregates", aggregate, node(1, table_cols=9), UNSUPPORTED, "node 1: AggregateExec with 9 aggregates (at most 8)"),
    ("aggregate: projection", aggregate, node(1, n_proj=1), INVALID, "node 1: AggregateExec takes no projection"),
    ("aggregate: nothing", aggregate, node(1, n_keys=0, table_cols=0), INVALID, "node 1: AggregateExec without group columns and aggregates"),
    ("aggregate: group column", aggregate, node(1, left_keys=(0, 5)), INVALID, "node 1: group column 5 out of range"),
    ("aggregate: list outside the pool", aggregate, node(1, table_slot=1), INVALID, "node 1: aggregate list outside the pool"),
    ("aggregate: COUNT of an expression", aggregate, pool(1, abi.AGG_INPUT_EXPR | 0), UNSUPPORTED, "node 1: aggregate 0: COUNT / COUNT DISTINCT over an expression"),
    ("aggregate: MIN", aggregate, pool(0, abi.AGG_MIN), UNSUPPORTED, "node 1: aggregate 0: MIN / MAX / SAMPLE / GROUP_CONCAT are not on the device"),
    ("aggregate: GROUP_CONCAT", aggregate, pool(0, abi.AGG_GROUP_CONCAT), UNSUPPORTED, "node 1: aggregate 0: MIN / MAX / SAMPLE / GROUP_CONCAT are not on the device"),
    ("aggregate: SUM DISTINCT", aggregate, pool(0, abi.AGG_SUM_DISTINCT), UNSUPPORTED, "node 1: aggregate 0: SUM / AVG with DISTINCT and COUNT(DISTINCT *) are not on the device"),
    ("aggregate: COUNT(DISTINCT *)", aggregate, pool(0, abi.AGG_COUNT_DISTINCT_STAR), UNSUPPORTED, "node 1: aggregate 0: SUM / AVG with DISTINCT and COUNT(DISTINCT *) are not on the device"),
    ("aggregate: unknown function", aggregate, pool(0, 99), INVALID, "node 1: aggregate 0: unknown function 99"),
    ("aggregate: input column", aggregate, pool(1, 7), INVALID, "node 1: aggregate 0 reads column 7 of 2"),
    ("aggregate: expression outside the pool", lambda: aggregate(abi.AGG_SUM, ENC_TV(col(1))), pool(1, abi.AGG_INPUT_EXPR | 3), INVALID,
     "node 1: aggregate 0: expression input at pool offset 3 of 4"),
    ("aggregate: expression outside the array", lambda: aggregate(abi.AGG_SUM, ENC_TV(col(1))), pool(3, 0), INVALID,
     "node 1: aggregate 0: expression outside the expression array"),
    ("aggregate: pattern op in an expression", lambda: aggregate(abi.AGG_SUM, ENC_TV(col(1))), expr(1, op=abi.EX_CONTAINS), UNSUPPORTED,
     "node 1: aggregate 0: REGEX / CONTAINS / STRSTARTS / STRENDS / LANGMATCHES in an aggregate's input expression"),
    ("aggregate: expression yields an id", lambda: aggregate(abi.AGG_SUM, ENC_TV(col(1))), pool(3, 1), INVALID,
     "node 1: aggregate 0: the input expression does not yield a typed value"),
    ("aggregate: not the root", aggregate_below_a_table, nothing, UNSUPPORTED, "node 1: an AggregateExec with aggregates must be the plan's root (node 2)"),
    ("input is an aggregate with aggregates", aggregate_with_a_consumer, nothing, UNSUPPORTED,
     "node 2: input 1 is an AggregateExec with aggregates, which must be the plan's root"),
    # projection, children
    ("projection: column", projection, pool(0, 9), INVALID, "ProjectionExec: projection column 9 out of range (2 columns)"),
    ("projection: outside the pool", projection, node(1, proj_off=1), INVALID, "ProjectionExec: projection outside the pool"),
    ("child: itself", projection, node(1, left=1), INVALID, "node 1: input child 1 must precede the node"),
    ("child: none", projection, node(1, left=-1), INVALID, "node 1: input child -1 must precede the node"),
    ("child: right of a join", hash_join, node(2, right=2), INVALID, "node 2: right child 2 must precede the node"),
    ("unknown kind", table, node(0, kind=77), INVALID, "node 0: unknown kind 77"),
    # the string table
    ("strings: pattern index", contains_filter, expr(2, u=5), INVALID, "expression: string pattern 5 out of range"),
    ("strings: one pattern, two functions", two_string_functions, expr(6, u=0), INVALID, "string pattern 0 is used by two different functions"),
    ("strings: a pattern on a store without strings", contains_filter, nothing, INVALID, "plan uses string functions but the store has no strings"),
    ("strings: STRLEN on a store without strings", strlen_filter, nothing, INVALID, "plan uses string functions but the store has no strings"),
    # ordering: two defects, the first one checked is the one reported
    ("order: two bad nodes, the lower index wins", union, both(node(0, table_cols=17), node(2, left=2)), UNSUPPORTED, "node 0: table with 17 columns"),
    ("order: two bad nodes, the lower index wins (swapped kinds)", hash_join, both(node(1, kind=77), node(2, n_keys=0)), INVALID, "node 1: unknown kind 77"),
    ("order: one node, the earlier check wins (join type before keys)", hash_join, node(2, join_type=9, n_keys=0), UNSUPPORTED, "node 2: join type 9"),
    ("order: one node, the earlier check wins (keys before fetch)", topk, node(1, n_keys=0, table_cols=0), UNSUPPORTED, "node 1: TopK with 0 sort keys"),
    ("order: the string table before a node", contains_filter, both(expr(2, u=5), node(0, table_cols=17)), INVALID, "expression: string pattern 5 out of range"),
    ("order: the store's strings before a node", strlen_filter, node(0, table_cols=17), INVALID, "plan uses string functions but the store has no strings"),
]

STRING_STORE_CASES = [
    ("strings: unsupported regex", long_regex, nothing, UNSUPPORTED, "string pattern 0: more than 64 positions"),
    ("order: an unsupported regex before a node", long_regex, node(0, table_cols=17), UNSUPPORTED, "string pattern 0: more than 64 positions"),
    # with strings on the store, the node's own defect is what is left
    ("strings present: the node is reported", strlen_filter, node(0, table_cols=17), UNSUPPORTED, "node 0: table with 17 columns"),
]


def compile_error(gs, build, spoil):
    pb, root = build()
    desc = pb.build(root)
    spoil(desc)
    with pytest.raises(rf.RdfGpuError) as e:
        gs.plan(desc)
    return e.value.status, str(e.value)


@pytest.mark.parametrize("name,build,spoil,status,text", CASES, ids=[c[0] for c in CASES])
def test_refusal(store, name, build, spoil, status, text):
    got = compile_error(store, build, spoil)
    assert got[0] == status and text in got[1], got


@pytest.mark.parametrize("name,build,spoil,status,text", STRING_STORE_CASES, ids=[c[0] for c in STRING_STORE_CASES])
def test_refusal_with_strings(store_with_strings, name, build, spoil, status, text):
    got = compile_error(store_with_strings, build, spoil)
    assert got[0] == status and text in got[1], got


def test_valid_plans_compile(store, store_with_strings):
    """The plans of the table compile as built: every refusal above is the broken field's (or, for the string functions, the store's)."""
    for build in (hash_join, cross_join, closure, union, table, topk, aggregate, projection, lambda: aggregate(abi.AGG_SUM, ENC_TV(col(1)))):
        pb, root = build()
        store.plan(pb.build(root))
    for build in (contains_filter, two_string_functions, strlen_filter):
        pb, root = build()
        store_with_strings.plan(pb.build(root))
