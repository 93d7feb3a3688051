"""Which forms of the multi-step cluster kernel can be launched, and at which bead count: a plain-Python restatement of the ACCEPTANCE
rules of cluster_plan (c3d_cluster.hip) and of the column layout of dev_model (c3d_config.cpp), for an unpartitioned MI355X (256 CUs, 8 XCDs,
every XCD in the launch's set).  The table is built from the acceptance rules alone: every case forces its geometry with the option
cluster_geometry, so what the planner would have preferred does not matter.  The cost model is restated beside it (planner_choice), only
to say which keys a problem reaches without the option.

A case is one (device potential, geometry, bead count, replicas, cluster_late_tiles); its key is what decides the code that runs:
(device potential, cw, rpw, nb, wl, nleft > 0, late, P > 1).  (potential, rpw, nb, wl, late) are the kernel's template arguments; cw, the
left-over columns and P > 1 are the run-time branches of the shared body (helper passes, left-over pass, the hand-off between parts).

tests/test_cluster_forms_table.py holds this file to itself and to the list of compiled forms; tests/test_gpu_cluster_forms.py runs
every case on the device and makes the library confirm each key.
"""
import functools
from collections import namedtuple

N_MIN, N_MAX = 9, 1024            # the smallest bead count the kernel tests of the suite use; cluster_plan refuses npad > 1024
CUS_PER_XCD, XCDS = 32, 8
HELPERS = 4

# {compute waves, rows per wave}: cluster_plan's list, every one with four helper waves and one workgroup per CU
GEOMETRIES = ((8, 1), (8, 2), (12, 2), (8, 4), (10, 4), (12, 4), (8, 3), (4, 2), (4, 4), (6, 4))
POTENTIALS = (0, 1, 2, 3, 4)

Key = namedtuple("Key", "pot cw rpw nb wl left late multi")
Case = namedtuple("Case", "key n nrep late_tiles why")


def geometry_option(cw, rpw, helpers=HELPERS):
    """the value of the option cluster_geometry"""
    return 100 * cw + 10 * rpw + helpers


def layout(n):
    """(npad, wl, nleft) of n beads with narrow_columns 1: lanes of the last 256-column block own wl consecutive columns, up to 8
    columns behind them are left over"""
    npad = (n + 255) // 256 * 256
    cols_last = n - (npad - 256)
    wl, nleft = cols_last // 64, cols_last % 64
    if wl == 0 or nleft > 8:
        wl, nleft = min(4, wl + 1), 0
    if npad > 1024:
        wl, nleft = 4, 0
    return npad, wl, nleft


def late_ok(pot, rpw, nb, wl):
    return pot >= 3 and rpw * (4 * (nb - 1) + wl) >= 6


def violations(pot, cw, rpw, n, nrep=3, late_tiles=1, helpers=HELPERS):
    """the names of all rules of cluster_plan that the forced geometry breaks, in cluster_plan's order"""
    npad, wl, nleft = layout(n)
    if npad > N_MAX:
        return ["npad"]
    if (cw, rpw) not in GEOMETRIES or helpers != HELPERS:
        return ["list"]
    nb, rw = npad // 256, cw * rpw
    out = []
    if rw % 8 or rw > 64:
        out.append("rows")
    if rpw * nb > 8:
        out.append("registers")
    if pot < 3 and (wl != 4 or nleft != 0):
        out.append("narrow")
    if nleft > 0 and (rw + 8 * (helpers - 1) - 1) // (8 * (helpers - 1)) > 4:
        out.append("leftover")
    P = (n + rw - 1) // rw
    per_xcd = (nrep + XCDS - 1) // XCDS
    if per_xcd * P > CUS_PER_XCD:
        out.append("parts")
    threads = (cw + helpers) * 64
    kumax = 3 if nb > 2 else 2
    if _late(pot, cw, rpw, nb, wl, P, late_tiles):
        if n > (threads - 64) * kumax:
            out.append("gather")
    elif n + 2 * ((n + 7) // 8) > threads * kumax:
        out.append("gather")
    return out


def refusal(pot, cw, rpw, n, nrep=3, late_tiles=1, helpers=HELPERS):
    """None where cluster_plan accepts the forced geometry, else the name of the first rule that refuses it"""
    v = violations(pot, cw, rpw, n, nrep, late_tiles, helpers)
    return v[0] if v else None


def _late(pot, cw, rpw, nb, wl, P, late_tiles):
    return bool(P > 1 and late_tiles != 0 and late_ok(pot, rpw, nb, wl)
                and (pot != 4 or ((cw + 3) // 4) * rpw * (4 * (nb - 1) + wl) >= 12))


def key_of(pot, cw, rpw, n, nrep=3, late_tiles=1):
    """the key of an accepted case, None for a refused one"""
    if refusal(pot, cw, rpw, n, nrep, late_tiles) is not None:
        return None
    npad, wl, nleft = layout(n)
    nb, P = npad // 256, (n + cw * rpw - 1) // (cw * rpw)
    return Key(pot, cw, rpw, nb, wl, nleft > 0, _late(pot, cw, rpw, nb, wl, P, late_tiles), P > 1)


def planner_choice(pot, n, nrep, late_tiles=1):
    """(cw, rpw) that cluster_plan itself chooses — its instruction-count model of one step, restated; the table's cases do not depend on
    it (they force their geometry): it says which keys a problem can reach WITHOUT cluster_geometry, and the device test of the refused
    geometries checks it where it hands the choice back to the planner.  None where no geometry is accepted."""
    npad, wl, _ = layout(n)
    nb = npad // 256
    best, choice = 1e30, None
    for cw, rpw in GEOMETRIES:                     # (the list's order decides between equal costs: the first one stays)
        if refusal(pot, cw, rpw, n, nrep, late_tiles) is not None:
            continue
        wps = (cw + 3) // 4
        per_slot = (rpw // 2) * 22.0 + (rpw & 1) * 19.0 if pot == 4 else rpw * 15.0
        valu = (1.6 if wps == 1 else 1.15 if wps == 2 else 1.0) * wps * ((4 * (nb - 1) + wl) * per_slot + 60.0)
        serial = 200.0 + ((140.0 + 0.92 * n) if parts(cw, rpw, n) > 1 else 0.0)
        if valu + serial < best:
            best, choice = valu + serial, (cw, rpw)
    return choice


@functools.lru_cache(maxsize=None)
def planner_keys():
    """the keys the planner's own choice reaches over every bead count, 1 .. 32 replicas on the fullest XCD and both settings of
    cluster_late_tiles"""
    # (replicas per XCD count through the parts they leave room for, 32 // per_xcd: one representative of each)
    reps = sorted({CUS_PER_XCD // (CUS_PER_XCD // p) for p in range(1, CUS_PER_XCD + 1)})
    out = set()
    for n in range(N_MIN, 768 + 1):                # (beyond 768 beads no geometry is accepted)
        for pot in POTENTIALS:
            for per_xcd in reps:
                for lt in (0, 1):
                    g = planner_choice(pot, n, XCDS * per_xcd, lt)
                    if g is not None:
                        out.add(key_of(pot, *g, n, XCDS * per_xcd, lt))
    return frozenset(out)


def parts(cw, rpw, n):
    return (n + cw * rpw - 1) // (cw * rpw)


@functools.lru_cache(maxsize=None)
def key_cases():
    """one case per key at the smallest bead count that realises it (3 replicas); cluster_late_tiles 0 only where the geometry would
    otherwise run late"""
    first = {}
    for n in range(N_MIN, N_MAX + 1):
        for pot in POTENTIALS:
            for cw, rpw in GEOMETRIES:
                for lt in (1, 0):
                    k = key_of(pot, cw, rpw, n, 3, lt)
                    if k is not None and k not in first:
                        first[k] = Case(k, n, 3, lt, "key")
    return tuple(first[k] for k in sorted(first))


@functools.lru_cache(maxsize=None)
def extra_cases():
    """per geometry, potentials 3 and 4: the left-over extremes nleft = 1, 7, 8 (n = 64 k + 1, + 7, + 8 in one block count: the
    smallest k the geometry takes all three at), and one case of 17 replicas (three on the fullest XCD) at the smallest bead count of
    the geometry's keys that three times its parts still fit"""
    out = []
    by_geom = {}
    for c in key_cases():
        by_geom.setdefault((c.key.pot, c.key.cw, c.key.rpw), []).append(c.n)
    for pot in (3, 4):
        for cw, rpw in GEOMETRIES:
            for k in range(1, 16):
                ns = [64 * k + r for r in (1, 7, 8)]
                if len({(n + 255) // 256 for n in ns}) == 1 and all(key_of(pot, cw, rpw, n) is not None and layout(n)[2] == r
                                                                    for n, r in zip(ns, (1, 7, 8))):
                    out += [Case(key_of(pot, cw, rpw, n), n, 3, 1, f"nleft{r}") for n, r in zip(ns, (1, 7, 8))]
                    break
            for n in sorted(set(by_geom.get((pot, cw, rpw), []))):
                k = key_of(pot, cw, rpw, n, 17, 1)
                if k is not None:
                    out.append(Case(k, n, 17, 1, "per_xcd3"))
                    break
            # (and the largest such bead count: the most parts per replica that three replicas on an XCD leave room for)
            for n in sorted(set(by_geom.get((pot, cw, rpw), [])), reverse=True):
                k = key_of(pot, cw, rpw, n, 17, 1)
                if k is not None:
                    out.append(Case(k, n, 17, 1, "per_xcd3_parts"))
                    break
    return tuple(out)


def cases(pot, cw, rpw):
    return [c for c in key_cases() + extra_cases() if (c.key.pot, c.key.cw, c.key.rpw) == (pot, cw, rpw)]


def template_forms(cs=None):
    """the (potential, rpw, nb, wl, late) tuples — template arguments of k_cluster / k_cluster_tp — that the cases launch"""
    return {(c.key.pot, c.key.rpw, c.key.nb, c.key.wl, c.key.late) for c in (key_cases() if cs is None else cs)}


# What cluster_plan must refuse: (variant of test_gpu_step_kernels.VARIANTS, cluster_geometry, beads, replicas, rule), the rule's name being
# what refusal() returns.  "list" cases are geometries cluster_plan does not hold, or a helper count it does not.  Two rules of
# cluster_plan appear nowhere: with the ten geometries of four helpers the left-over passes per chain helper are at most three
# (64 rows / 24) and the gather's units per thread stay below the bound (at most 640 of 1024 up to 512 beads, 960 of 1536 up to 768; beyond
# 768 "registers" or "parts" has refused already) — they are invariants of the list, not rules that refuse a problem
# (tests/test_cluster_forms_table.py holds that).
REFUSED = (
    # potentials 0-2 off the full last block: narrow blocks (wl 1..3) and left-over columns
    ("pot0", 824, 64, 3, "narrow"), ("pot1", 1224, 130, 3, "narrow"), ("pot2", 844, 200, 3, "narrow"), ("pot0", 1244, 257, 3, "narrow"),
    ("pot1", 824, 455, 3, "narrow"), ("pot2", 1224, 520, 3, "narrow"), ("pot0", 424, 585, 3, "narrow"),
    # targets in registers: rpw * nb > 8
    ("shipped", 1244, 513, 3, "registers"), ("pot3_clamp", 844, 520, 3, "registers"), ("shipped", 834, 769, 3, "registers"),
    ("pot1", 644, 760, 3, "registers"), ("shipped", 444, 700, 3, "registers"), ("pot3_clamp", 1044, 1000, 3, "registers"),
    ("pot3_clamp", 834, 1024, 3, "registers"),
    # more parts than the XCD has CUs: one replica's, and three replicas' on the fullest XCD
    ("shipped", 814, 257, 3, "parts"), ("pot0", 814, 512, 3, "parts"), ("pot3_clamp", 424, 264, 3, "parts"), ("shipped", 824, 513, 3, "parts"),
    ("shipped", 1224, 769, 3, "parts"), ("pot3_clamp", 1224, 1024, 3, "parts"), ("pot0", 1224, 1024, 3, "parts"),
    ("shipped", 844, 400, 17, "parts"), ("pot3_clamp", 1224, 265, 17, "parts"), ("pot2", 444, 250, 17, "parts"),
    # not in the list
    ("shipped", 744, 37, 3, "list"), ("shipped", 1242, 455, 3, "list"), ("pot3_clamp", 1624, 250, 3, "list"), ("pot1", 1234, 250, 3, "list"),
    ("shipped", 614, 120, 3, "list"), ("pot2", 822, 250, 3, "list"),
)
VARIANT_POT = {"shipped": 4, "pot0": 0, "pot1": 1, "pot2": 2, "pot3_clamp": 3, "pot3_rs1": 3}


def refused_rule(variant, geom, n, nrep):
    """the rule by which this file says cluster_plan refuses a REFUSED entry (None: it would be accepted)"""
    cw, rpw, nh = geom // 100, geom // 10 % 10, geom % 10
    assert cw > 0                  # (cluster_plan reads "no geometry forced" from cw == 0)
    return refusal(VARIANT_POT[variant], cw, rpw, n, nrep, 1, nh)
