"""tests/cluster_forms.py held to itself and to the list of compiled forms (no GPU).

Counts of the table (256 CUs, 8 XCDs, 3 replicas, 9 .. 1024 beads):
  keys (device potential, cw, rpw, nb, wl, nleft > 0, late, P > 1): 538 — potential 4: 238, potential 3: 243, potentials 0, 1, 2: 19 each —
    at 26 bead counts: 9, 17, 25, 33, 41, 49, 65, 73, 129, 137, 193, 201, 257, 321, 329, 385, 393, 449, 457, 513, 577, 585, 641, 649, 705, 713;
    199 of them need cluster_late_tiles 0 (the geometry would run late otherwise);
  further cases: 60 left-over extremes (nleft 1, 7, 8 at 65, 71, 72 beads: every geometry, potentials 3 and 4) and 40 of 17 replicas
    (three on the fullest XCD: per geometry at 9 beads and at the most parts that still fit, 73 .. 457 beads);
  template forms <potential, rpw, nb, wl, late> compiled: 210 per kernel — 87 each for potentials 3 and 4, 12 each for potentials 0, 1, 2;
  launchable: 136 — 56 each for potentials 3 and 4, 8 each for potentials 0, 1, 2;
  never launchable: 74 — rpw 1 at nb >= 2 (55 forms: P = n / 8 > 32 parts) and every nb 4 form (38, 19 of them in both families:
    beyond 768 beads only rpw 1 and 2 keep their targets in registers, and 8 or 24 rows a part need more than 32 parts).
Reached by the planner's own choice (its cost model restated: cluster_forms.planner_choice; any bead count, 1 .. 32 replicas on the
fullest XCD, either setting of cluster_late_tiles): 290 of the 538 keys and 99 of the 136 forms — potential 4: 128 keys, 38 forms;
potential 3: 132, 43; potentials 0, 1, 2: 10, 6 each.  The other 248 keys and 37 forms run only under a forced geometry: for the shipped
potential every 8 x 1 and 6 x 4 key, 8 x 3 beyond 72 beads (a last block of one column a lane), and most keys of a geometry away from the sizes the
model prefers it at.
Two of cluster_plan's rules refuse nothing: the left-over passes per chain helper and the gather's units per thread hold for each of the
ten geometries at every bead count another rule lets through (test_two_rules_refuse_nothing).
"""
from collections import Counter

from tests import cluster_forms as cf

# for_each_cluster_form (c3d_cluster.hip), transcribed: its twelve (RPW, NB) pairs; WL = 4 for every potential and 3, 2, 1 for potentials
# 3 and 4; LATE = false always and LATE = true where cluster_late_ok
PAIRS = ((1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (4, 1), (4, 2))


def compiled_forms():
    out = set()
    for pot in range(5):
        for rpw, nb in PAIRS:
            for wl in ((4, 3, 2, 1) if pot >= 3 else (4,)):
                out.add((pot, rpw, nb, wl, False))
                if pot >= 3 and rpw * (4 * (nb - 1) + wl) >= 6:
                    out.add((pot, rpw, nb, wl, True))
    return out


def test_counts():
    kc = cf.key_cases()
    assert len(kc) == 538 and len({c.key for c in kc}) == 538
    assert Counter(c.key.pot for c in kc) == {4: 238, 3: 243, 0: 19, 1: 19, 2: 19}
    assert sorted({c.n for c in kc}) == [9, 17, 25, 33, 41, 49, 65, 73, 129, 137, 193, 201, 257, 321, 329, 385, 393, 449, 457, 513, 577,
                                         585, 641, 649, 705, 713]
    assert sum(c.late_tiles == 0 for c in kc) == 199
    assert sum(c.key.pot == 2 and c.key.nb >= 2 for c in kc) == 9       # the keys whose oracle comparison ends at step 22
    ex = cf.extra_cases()
    assert Counter(c.why for c in ex) == {"nleft1": 20, "nleft7": 20, "nleft8": 20, "per_xcd3": 20, "per_xcd3_parts": 20}
    assert Counter(f[0] for f in compiled_forms()) == {0: 12, 1: 12, 2: 12, 3: 87, 4: 87}


def test_every_key_is_realised_at_its_bead_count_and_not_one_bead_earlier():
    for c in cf.key_cases():
        k = c.key
        assert cf.violations(k.pot, k.cw, k.rpw, c.n, c.nrep, c.late_tiles) == [], c
        assert cf.key_of(k.pot, k.cw, k.rpw, c.n, c.nrep, c.late_tiles) == k, c
        assert c.late_tiles == 1 or cf.key_of(k.pot, k.cw, k.rpw, c.n, c.nrep, 1) != k, c      # late tiles forbidden only where needed
        if c.n > cf.N_MIN:
            assert all(cf.key_of(k.pot, k.cw, k.rpw, c.n - 1, c.nrep, lt) != k for lt in (0, 1)), c
    # every key that any bead count realises is in the table
    seen = {cf.key_of(pot, cw, rpw, n, 3, lt) for n in range(cf.N_MIN, cf.N_MAX + 1) for pot in cf.POTENTIALS for cw, rpw in cf.GEOMETRIES
            for lt in (0, 1)} - {None}
    assert seen == {c.key for c in cf.key_cases()}


def test_further_cases_are_what_they_claim():
    by = {}
    for c in cf.extra_cases():
        k = c.key
        assert k.pot in (3, 4) and cf.key_of(k.pot, k.cw, k.rpw, c.n, c.nrep, c.late_tiles) == k, c
        by.setdefault((k.pot, k.cw, k.rpw), []).append(c)
    assert len(by) == 20
    for cs in by.values():
        left = {c.why: c.n for c in cs if c.why.startswith("nleft")}
        assert {w: cf.layout(n)[2] for w, n in left.items()} == {"nleft1": 1, "nleft7": 7, "nleft8": 8}
        assert len({cf.layout(n)[0] for n in left.values()}) == 1 and {n % 64 for n in left.values()} == {1, 7, 8}
        for c in cs:
            if c.why.startswith("per_xcd3"):
                assert c.nrep == 17 and 3 * cf.parts(c.key.cw, c.key.rpw, c.n) <= 32
        assert any(c.why == "per_xcd3_parts" and c.key.multi for c in cs)


def test_launchable_forms_are_compiled_and_the_rest_are_the_two_families():
    compiled, launchable = compiled_forms(), cf.template_forms()
    assert len(compiled) == 210 and len(launchable) == 136
    assert Counter(f[0] for f in launchable) == {3: 56, 4: 56, 0: 8, 1: 8, 2: 8}
    assert launchable <= compiled
    never = compiled - launchable
    assert never == {f for f in compiled if (f[1] == 1 and f[2] >= 2) or f[2] == 4}
    # and at any replica count: more replicas only tighten the parts rule, the other rules do not see them
    assert cf.template_forms(cf.key_cases() + cf.extra_cases()) == launchable


def test_two_rules_refuse_nothing():
    """cluster_plan's left-over-pass rule and its gather bound are never the reason a listed geometry is refused, nor even broken together
    with another rule: REFUSED can hold no case of them"""
    for n in range(cf.N_MIN, cf.N_MAX + 1):
        for pot in (0, 3, 4):
            for cw, rpw in cf.GEOMETRIES:
                for nrep in (1, 17, 64):
                    for lt in (0, 1):
                        v = cf.violations(pot, cw, rpw, n, nrep, lt)
                        assert "leftover" not in v and "gather" not in v and "rows" not in v, (pot, cw, rpw, n, nrep, lt, v)


def test_refused_list_draws_from_every_rule_that_can_refuse():
    assert 25 <= len(cf.REFUSED) <= 35
    for variant, geom, n, nrep, rule in cf.REFUSED:
        assert cf.refused_rule(variant, geom, n, nrep) == rule, (variant, geom, n, nrep)
    assert {r[4] for r in cf.REFUSED} == {"narrow", "registers", "parts", "list"}
    assert {r[3] for r in cf.REFUSED} == {3, 17}


def test_what_the_planner_reaches_on_its_own():
    keys = cf.planner_keys()
    assert keys <= {c.key for c in cf.key_cases()}
    assert Counter(k.pot for k in keys) == {4: 128, 3: 132, 0: 10, 1: 10, 2: 10}
    forms = {(k.pot, k.rpw, k.nb, k.wl, k.late) for k in keys}
    assert Counter(f[0] for f in forms) == {4: 38, 3: 43, 0: 6, 1: 6, 2: 6}
    shipped = {(k.cw, k.rpw) for k in keys if k.pot == 4}
    assert shipped == set(cf.GEOMETRIES) - {(8, 1), (6, 4)}
    assert {(k.nb, k.wl) for k in keys if k.pot == 4 and k.rpw == 3} == {(1, 1)}       # 8 x 3: up to 72 beads only
    # the choices the documents record: chr21_1mb (37 beads) x 4 and x 20, chr1_500kb (455) x 20, chr4_1mb (192) x 20
    assert cf.planner_choice(4, 37, 4) == (4, 2) and cf.parts(4, 2, 37) == 5
    assert cf.planner_choice(4, 37, 20)[1] == 2
    assert cf.planner_choice(4, 455, 20) == (12, 4) and cf.parts(12, 4, 455) == 10
    assert cf.planner_choice(4, 1000, 3) is None and cf.planner_choice(0, 455, 3) is None
