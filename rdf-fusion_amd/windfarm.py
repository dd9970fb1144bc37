"""A Wind Farm-shaped store and the GroupedProduction plan (the reference's third workload: bench/tests/plans/wind_farm.rs, snapshots
`Wind Farm - GroupedProduction1..4 (Execution Plan).snap`, over the chrontext `rds_power` model).

Shape: sites with a label; per site turbines, each reached through a functional aspect that carries the turbine's label; per turbine a
generator system and a generator, one functional-aspect hop each; per generator a "Production" time series (and a second series that the
plan's label pattern leaves out); per series data points with `hasValue` (xsd:integer here, so that AVG is exact) and `hasTimestamp`
(xsd:dateTime).  The turbines of a site take turns in how their timestamps are written: UTC (`Z`), an offset of +05:30, no timezone — the
typed-value rows carry the UTC instant, the presence bit and `tz_minutes`, as a host fills them.  Everything is numpy; ids are dense from
1; default graph only.

The plan is the snapshot's: the join tree, the dateTime range FILTER on the timestamp pattern, ONE ProjectionExec with the five date-part
programs and the 7-key AVG.  The reference computes `ENC_TV(t) as __common_expr` once and reads it from three projections; a
dateTime-valued computed column has no 24-byte record here, so every program inlines ENC_TV(t)."""
from dataclasses import dataclass, field

import numpy as np

from . import abi, xsd
from .engine import TV_DTYPE
from .plan import (PlanBuilder, quad_pattern, col, lit_tv, integer, decimal, date_time, ENC_TV, EBV, EQ, GEQ, LEQ, AND, MUL, DIV, FLOOR,
                   YEAR, MONTH, DAY, HOURS, MINUTES)

PREDICATES = ["rdf:type", "rdfs:label", "rds:hasFunctionalAspect", "rds:hasFunctionalAspectNode", "ct:hasTimeseries", "ct:hasDataPoint",
              "ct:hasValue", "ct:hasTimestamp"]
CLASSES = ["rds:Site", "rds:A", "rds:RA", "rds:GAA"]
SITE_LABELS = ["Wind Mountain", "Gale Ridge", "Storm Coast", "Breeze Valley"]
OFFSETS = (0, 330, None)          # a turbine's timestamps: UTC, +05:30, no timezone — in turn
STEP_SECONDS = 300                # between the data points of a series


@dataclass
class WindFarmDataset:
    g: np.ndarray
    s: np.ndarray
    p: np.ndarray
    o: np.ndarray
    typed_values: np.ndarray          # TV_DTYPE, index = object id
    decimals: np.ndarray              # (n, 2) int64: the i128 of the timestamps
    pred: dict
    cls: dict
    labels: dict                      # text -> object id of the string literal
    n_ids: int
    first_local: str                  # the local time of every series' first data point
    counts: dict = field(default_factory=dict)


def generate(points_per_series=700, n_sites=2, turbines_per_site=3, first_local="2022-08-31T19:00:00", seed=0):
    """`points_per_series` data points per Production series, STEP_SECONDS apart from `first_local` (local time of the turbine's offset): the
    default 700 x 300 s run 58 h, across the end of August."""
    rng = np.random.default_rng(seed)
    next_id = [1]

    def take(n):
        b = next_id[0]
        next_id[0] += int(n)
        return b
    pred = {n: take(1) for n in PREDICATES}
    cls = {n: take(1) for n in CLASSES}
    T = n_sites * turbines_per_site
    turbine_labels = [f"A{k + 1}" for k in range(turbines_per_site)]
    texts = SITE_LABELS[:n_sites] + turbine_labels + ["Production", "WindSpeed"]
    labels = {t: take(1) for t in texts}
    site = take(n_sites) + np.arange(n_sites)
    wtur_asp, wtur, gensys_asp, gensys, gen_asp, gen = (take(T) + np.arange(T) for _ in range(6))
    ts_prod, ts_other = take(T) + np.arange(T), take(T) + np.arange(T)
    n_other = max(1, points_per_series // 7)
    n_dp = T * (points_per_series + n_other)
    dp = take(n_dp) + np.arange(n_dp)
    val_base = take(1000)                                   # xsd:integer 0..999
    t_base = take(n_dp)                                     # one dateTime literal per data point
    n_ids = next_id[0]

    S, P, O = [], [], []

    def emit(s, p, o):
        s = np.asarray(s, dtype=np.uint32)
        S.append(s)
        P.append(np.full(len(s), p, dtype=np.uint32))
        O.append(np.broadcast_to(np.asarray(o, dtype=np.uint32), s.shape) if np.ndim(o) == 0 else np.asarray(o, dtype=np.uint32))
    ty, lab, fa, fan = pred["rdf:type"], pred["rdfs:label"], pred["rds:hasFunctionalAspect"], pred["rds:hasFunctionalAspectNode"]
    site_of = np.repeat(np.arange(n_sites), turbines_per_site)
    emit(site, ty, cls["rds:Site"])
    emit(site, lab, [labels[t] for t in SITE_LABELS[:n_sites]])
    emit(site[site_of], fa, wtur_asp)
    emit(wtur_asp, lab, [labels[turbine_labels[k % turbines_per_site]] for k in range(T)])
    emit(wtur, fan, wtur_asp)
    emit(wtur, ty, cls["rds:A"])
    emit(wtur, fa, gensys_asp)
    emit(gensys, fan, gensys_asp)
    emit(gensys, ty, cls["rds:RA"])
    emit(gensys, fa, gen_asp)
    emit(gen, fan, gen_asp)
    emit(gen, ty, cls["rds:GAA"])
    emit(gen, pred["ct:hasTimeseries"], ts_prod)
    emit(gen, pred["ct:hasTimeseries"], ts_other)
    emit(ts_prod, lab, labels["Production"])
    emit(ts_other, lab, labels["WindSpeed"])
    # data points: the Production series of turbine k, then its other series
    series = np.concatenate([np.repeat(ts_prod, points_per_series), np.repeat(ts_other, n_other)])
    turbine = np.concatenate([np.repeat(np.arange(T), points_per_series), np.repeat(np.arange(T), n_other)])
    index = np.concatenate([np.tile(np.arange(points_per_series), T), np.tile(np.arange(n_other), T)])
    emit(series, pred["ct:hasDataPoint"], dp)
    emit(dp, pred["ct:hasValue"], val_base + rng.integers(0, 1000, n_dp))
    emit(dp, pred["ct:hasTimestamp"], t_base + np.arange(n_dp))

    s, p, o = np.concatenate(S), np.concatenate(P), np.concatenate(O)
    tv = np.zeros(n_ids, dtype=TV_DTYPE)
    tv["tag"][1:] = abi.TV_NAMED_NODE
    tv["lo"][1:] = np.arange(1, n_ids)
    order = {t: r for r, t in enumerate(sorted(texts))}
    for t, i in labels.items():
        tv[i] = (order[t], 0, abi.TV_STRING, 0, 0)
    tv["tag"][val_base:val_base + 1000] = abi.TV_INTEGER
    tv["lo"][val_base:val_base + 1000] = np.arange(1000)
    # timestamps: the local time first_local + STEP_SECONDS * index, written with the turbine's offset; the value is the UTC instant
    local0 = xsd.parse_date_time(first_local)[0] // xsd.SCALE
    tz = [OFFSETS[k % len(OFFSETS)] for k in range(T)]
    dec = np.zeros((n_dp, 2), np.int64)
    for j in range(n_dp):
        off = tz[turbine[j]]
        v = (local0 + STEP_SECONDS * int(index[j]) - 60 * (off or 0)) * xsd.SCALE
        dec[j] = (v & ((1 << 63) - 1) | -(v & (1 << 63)), v >> 64)
        tv[t_base + j] = (j, 0 if off is None else 1, abi.TV_DATE_TIME, 0, off or 0)
    counts = {"sites": n_sites, "turbines": T, "data_points": n_dp, "production_points": T * points_per_series, "triples": len(s)}
    return WindFarmDataset(np.zeros(len(s), np.uint32), s, p, o, tv, dec, pred, cls, labels, n_ids, first_local, counts)


def _join(pb, left, right, keep):
    """the inner hash join of two inputs on the variables they share, projected to the columns named `keep`"""
    ln, rn = pb.names[left], pb.names[right]
    on = [(ln.index(v), rn.index(v)) for v in ln if v in rn]
    return pb.hash_join(left, right, on, projection=[ln.index(k) if k in ln else len(ln) + rn.index(k) for k in keep])


def minute_10(tv):
    """`MUL(9:10, FLOOR(DIV(MINUTES(tv), 10.0))) as minute_10`: the 10-minute bucket, an xsd:decimal"""
    return MUL(integer(10), FLOOR(DIV(MINUTES(tv), decimal(10 * xsd.SCALE))))


def grouped_production(ds, site_label="Wind Mountain", turbine_label=None, t_from=None, t_to=None):
    """(PlanBuilder, root) of `Wind Farm - GroupedProduction`: AVG(val) per (site_label, wtur_label, year, month, day, hour, minute_10)
    over the Production series of the site's turbines (of the one labelled `turbine_label`, if given) between two dateTimes without a
    timezone, as the snapshots' literals are (`10:{value:..,offset:}`; None: no FILTER).  Output columns: the seven keys, then avg_val.
    Build with `pb.build(root, agg_columns=True, value_keys=True)`."""
    pr, cl, pb = ds.pred, ds.cls, PlanBuilder()
    src = lambda s, p, o: pb.data_source(quad_pattern(s, p, o))
    is_label = lambda text: EBV(EQ(ENC_TV(col(1)), lit_tv(abi.TV_STRING, int(ds.typed_values["lo"][ds.labels[text]]))))
    ty, lab, fa, fan = pr["rdf:type"], pr["rdfs:label"], pr["rds:hasFunctionalAspect"], pr["rds:hasFunctionalAspectNode"]
    sl, wl = "site_label", "wtur_label"
    n = _join(pb, src("site", ty, cl["rds:Site"]), pb.filter(src("site", lab, sl), is_label(site_label)), ["site", sl])
    n = _join(pb, n, src("site", fa, "wtur_asp"), [sl, "wtur_asp"])
    turbine = src("wtur_asp", lab, wl)
    n = _join(pb, n, turbine if turbine_label is None else pb.filter(turbine, is_label(turbine_label)), [sl, "wtur_asp", wl])
    n = _join(pb, n, src("wtur", fan, "wtur_asp"), [sl, wl, "wtur"])
    n = _join(pb, n, src("wtur", fa, "gensys_asp"), [sl, wl, "wtur", "gensys_asp"])
    n = _join(pb, n, src("wtur", ty, cl["rds:A"]), [sl, wl, "gensys_asp"])
    n = _join(pb, n, src("gensys", fan, "gensys_asp"), [sl, wl, "gensys"])
    n = _join(pb, n, src("gensys", ty, cl["rds:RA"]), [sl, wl, "gensys"])
    n = _join(pb, n, src("gensys", fa, "generator_asp"), [sl, wl, "generator_asp"])
    n = _join(pb, n, src("generator", fan, "generator_asp"), [sl, wl, "generator"])
    n = _join(pb, n, src("generator", ty, cl["rds:GAA"]), [sl, wl, "generator"])
    n = _join(pb, n, src("generator", pr["ct:hasTimeseries"], "ts"), [sl, wl, "ts"])
    n = _join(pb, n, src("ts", lab, ds.labels["Production"]), [sl, wl, "ts"])
    n = _join(pb, n, src("ts", pr["ct:hasDataPoint"], "dp"), [sl, wl, "dp"])
    n = _join(pb, n, src("dp", pr["ct:hasValue"], "val"), [sl, wl, "dp", "val"])
    stamps = src("dp", pr["ct:hasTimestamp"], "t")
    if t_from is not None:
        t = ENC_TV(col(1))
        stamps = pb.filter(stamps, AND(EBV(GEQ(t, date_time(xsd.parse_date_time(t_from)[0], False))), EBV(LEQ(t, date_time(xsd.parse_date_time(t_to)[0], False)))))
    n = _join(pb, n, stamps, [sl, wl, "val", "t"])
    tv = ENC_TV(col(3))
    x = pb.extend(n, [minute_10(tv), HOURS(tv), DAY(tv), MONTH(tv), YEAR(tv)], keep=[0, 1, 2], names=["minute_10", "hour", "day", "month", "year"])
    root = pb.aggregate(x, [0, 1, 7, 6, 5, 4, 3], [(abi.AGG_AVG, 2)])
    pb.names[root][-1] = "avg_val"
    return pb, root
