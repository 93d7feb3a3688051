"""One pair's coefficient and energy per potential, restated in numpy float64 from the statements of oracle/c3d_oracle.c (softsq,
c3o_energy_force) — a second text of the same model, dense over a replica's n x n pairs.  It supplies what the oracle does not: every
row's TERM SCALES, from which tests/test_gpu_pair_table.py forms the bound of a force component before anything runs, and it takes the
MUTATIONS with which tests/test_pair_cases.py shows that the tables of tests/pair_cases.py can tell a wrong pair term from a right one.

Term scales (the size of what is rounded, not of what is left after cancellation), per pair and per unit of the coordinate difference:
  NOE             2 w S (d + t) / d      the coefficient is -w S g / d with |g| <= 2 |d - t| <= 2 (d + t) in every branch of the tables'
                                         models: g = 2 (d - t) in the square part, and every tail starts at the square's value at its
                                         switch and grows, if at all, by less than 2 per A (gen0, the steepest: from 4 at the switch
                                         towards 6, slope 2 b / D^3 <= 2 beyond it); d + t covers the cancellation in d - t
  repel           4 w_vdw k_rep R^2      R = repel_s r0_rep; only where the oracle's term acts (r^2 < R^2): beyond R the kernels' clamp
                                         returns an exact 0
  take-back       4 w_vdw k_rep R^2      once more for a neighbour closer than rep_sep inside R: the pair loop adds the term, the chain
                                         pass takes it back out in another rounding
  bond / angle    2 w k (d + r0) / d
A component's bound is sum over the row's terms of scale |x_ic - x_jc| (B eps + guard), guard = min(1, g / (2 r^2)) on the NOE and repel
terms: the fp32 pair loop adds g = 1e-12 to r^2 inside its fma chain where the oracle clamps r^2 at 1e-12 (fp64: g = 1e-30)."""
import numpy as np

MUTATIONS = ("clamp_wrong_side", "rs_mrs_swapped", "lower_exponent_2_for_3", "masym_ignored", "tail_sign_pot0", "no_take_back",
             "take_back_at_rep_sep", "angle_on_above_a0", "unrestrained_weight_on", "guard_dropped", "min_sep_ignored", "radius_without_repel_s")

FIELDS = ("min_sep", "noe_pot", "rep_sep", "ang_mode", "s_noe", "rswitch", "asym", "masym", "mrswitch", "k_bond", "b0", "k_ang", "a0", "r0_rep",
          "k_rep", "msoexp")


def params_from(m):
    """the model's numbers as the oracle holds them: the float32 fields of a c3d_model widened (msoexp 0 = the default, 2)"""
    P = {k: (int(getattr(m, k)) if k in ("min_sep", "noe_pot", "rep_sep", "ang_mode", "msoexp") else float(getattr(m, k))) for k in FIELDS}
    if P["msoexp"] == 0:
        P["msoexp"] = 2
    return P


def softsq(P, delta, mut=None):
    """(dE/d delta, E, branch) of the NOE term without S and w, elementwise.  Branches: 0 square, 1 upper tail, 2 lower tail of potential 0
    (the mirrored upper one), 3 lower soft side of potential 3."""
    delta = np.asarray(delta, dtype=np.float64)
    rs, mrs = P["rswitch"], P["mrswitch"]
    if mut == "rs_mrs_swapped":
        rs, mrs = mrs, rs
    pot = P["noe_pot"]
    ad = np.abs(delta)
    c = P["asym"] * rs
    b = (c - 2.0 * rs) * rs * rs
    a = rs * rs - b / rs - c * rs
    up = delta < -rs if mut == "clamp_wrong_side" else delta > rs
    if pot == 0:
        soft = ad > rs
    elif pot in (1, 3):
        soft = up
    else:
        soft = np.zeros(delta.shape, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g_tail = -b / (ad * ad) + c
        e_tail = a + b / ad + c * ad
        g = np.where(soft, np.where(delta > 0, g_tail, g_tail if mut == "tail_sign_pot0" else -g_tail), 2.0 * delta)
        e = np.where(soft, e_tail, delta * delta)
        branch = np.where(soft, np.where(delta > 0, 1, 2), 0)
        if pot == 3:
            mc = 0.0 if mut == "masym_ignored" else P["masym"]
            low = delta < -mrs
            if P["msoexp"] == 2:
                mb = (mc - 2.0 * mrs) * mrs * mrs * mrs / 2.0
                ma = mrs * mrs - mb / (mrs * mrs) - mc * mrs
                e_low = ma + mb / (ad * ad) + mc * ad
                g_low = -(-2.0 * mb / (ad * ad if mut == "lower_exponent_2_for_3" else ad * ad * ad) + mc)
            else:
                mb = (mc - 2.0 * mrs) * mrs * mrs
                ma = mrs * mrs - mb / mrs - mc * mrs
                e_low = ma + mb / ad + mc * ad
                g_low = -(-mb / (ad * ad) + mc)
            g, e, branch = np.where(low, g_low, g), np.where(low, e_low, e), np.where(low, 3, branch)
    return g, e, branch


def energy_force(P, t10, x, w_all=1.0, w_vdw=1.0, repel_s=1.0, mut=None, guard=0.0):
    """A replica's forces [n, 3], energies (NOE, bond + angle, repel: unweighted, as the oracle's), and what the tables ask about its rows:
    `scale` [n, 3] = sum of the row's term scales times |x_ic - x_jc| (guard share included as scale x min(1, guard / (2 r^2)) in
    `guard_part`), `abs_e` = the sums of |energy terms|, `branch` [n, n] the NOE branch of every restrained pair (-1: none)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    t10 = np.asarray(t10)
    dv = x[:, None, :] - x[None, :, :]
    r2raw = dv[..., 0] * dv[..., 0] + dv[..., 1] * dv[..., 1] + dv[..., 2] * dv[..., 2]
    r2 = r2raw if mut == "guard_dropped" else np.maximum(r2raw, 1e-12)
    idx = np.arange(n)
    sep = np.abs(idx[:, None] - idx[None, :])
    off = sep > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.sqrt(r2)
        coef = np.zeros((n, n))
        scale = np.zeros((n, n))
        # NOE
        restrained = off & (t10 > 0 if mut != "unrestrained_weight_on" else np.ones((n, n), dtype=bool))
        if mut != "min_sep_ignored":
            restrained &= sep >= P["min_sep"]
        t = np.where(t10 > 0, 0.1 * t10, 0.0)
        g, e, br = softsq(P, d - t, mut)
        coef = np.where(restrained, coef - w_all * P["s_noe"] * g / d, coef)
        s_noe = np.where(restrained, 2.0 * w_all * P["s_noe"] * (d + t) / d, 0.0)
        e_noe = np.where(restrained, P["s_noe"] * e, 0.0)
        branch = np.where(restrained, br, -1)
        # bond
        bond = sep == 1
        coef = np.where(bond, coef - w_all * 2.0 * P["k_bond"] * (d - P["b0"]) / d, coef)
        s_chain = np.where(bond, 2.0 * w_all * P["k_bond"] * (d + P["b0"]) / d, 0.0)
        e_chain = np.where(bond, P["k_bond"] * (d - P["b0"]) ** 2, 0.0)
        # repel
        R = (P["r0_rep"] if mut == "radius_without_repel_s" else repel_s * P["r0_rep"])
        R2 = R * R
        lo = 1 if mut == "no_take_back" else (P["rep_sep"] + 1 if mut == "take_back_at_rep_sep" else P["rep_sep"])
        rep = (sep >= lo) & (r2 < R2)
        coef = np.where(rep, coef + w_vdw * P["k_rep"] * 4.0 * (R2 - r2), coef)
        inside = off & (r2 < R2)                       # the pair loop's term acts here; below rep_sep the chain pass takes it back
        s_rep = np.where(inside, 4.0 * w_vdw * P["k_rep"] * R2 * np.where(sep < P["rep_sep"], 2.0, 1.0), 0.0)
        e_rep = np.where(rep, P["k_rep"] * (R2 - r2) ** 2, 0.0)
        # angle
        ang = (sep == 2) & (P["k_ang"] > 0)
        if P["ang_mode"] != 1 and mut != "angle_on_above_a0":
            ang &= r2 < P["a0"] * P["a0"]
        coef = np.where(ang, coef - w_all * 2.0 * P["k_ang"] * (d - P["a0"]) / d, coef)
        s_chain = s_chain + np.where(ang, 2.0 * w_all * P["k_ang"] * (d + P["a0"]) / d, 0.0)
        e_chain = e_chain + np.where(ang, P["k_ang"] * (d - P["a0"]) ** 2, 0.0)
        F = (coef[..., None] * dv).sum(1)
        adv = np.abs(dv)
        gshare = np.minimum(1.0, guard / (2.0 * r2)) if guard else np.zeros((n, n))
        scale = ((s_noe + s_rep + s_chain)[..., None] * adv).sum(1)
        guard_part = (((s_noe + s_rep) * gshare)[..., None] * adv).sum(1)
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    energies = (float(e_noe[up].sum()), float(e_chain[up].sum()), float(e_rep[up].sum()))
    abs_e = (float(np.abs(e_noe[up]).sum()), float(np.abs(e_chain[up]).sum()), float(np.abs(e_rep[up]).sum()))
    return dict(F=F, e=energies, abs_e=abs_e, scale=scale, guard_part=guard_part, branch=branch, coef=coef,
                taken_back=inside & (sep < P["rep_sep"]), rep=rep, ang=ang, r2=r2raw)


# unit roundoffs, and B of the fp32 forms from the count of roundings (profiles/r34_pair_table.md has the count form by form: at most 24, rounded up to 32)
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
B32 = 32.0
GUARD32, GUARD64 = 1e-12, 1e-30
F64_CAP = 1e-11           # the suite's fp64 force cap (tests/test_gpu_f64_boundary.py: 1e-10 |F| + 1e-11 max|F|), here on a row's own scale


def force_bound(ref, precision):
    """[n, 3]: the bound of every force component of a replica evaluated by energy_force(..., guard=GUARD32 | GUARD64)"""
    if precision == 32:
        return B32 * EPS32 * ref["scale"] + ref["guard_part"]
    return F64_CAP * ref["scale"] + ref["guard_part"]
