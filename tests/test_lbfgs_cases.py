"""The L-BFGS controller cases of tests/lbfgs_cases.py, admitted on the CPU: jointly they take every branch the list in
test_cases_take_every_branch names, the float32 twin of the restatement takes the same branch on every step and ends within a quarter
of the GPU bound, every discontinuous decision has a margin, and every mutation of lbfgs_ref.MUTATIONS ends at least ten GPU bounds
from the restatement at some checkpoint of some case.  tests/test_gpu_lbfgs_controller.py runs the same table on the device: what is
proved here is what makes a pass there mean something."""
import numpy as np
import pytest

from tests import lbfgs_cases as T
from tests import lbfgs_ref as L


def _logs():
    return [(name, n, slot, T.reference(name, n, slot)[1]) for name, n in T.CASE_SIZES for slot in (0, 1)]


def test_restatement_keeps_its_bits_and_counts_resets(built):
    """lbfgs_run with a log is the lbfgs_run the suite had: the same statements on the unmutated path (spelt out here once more, without
    log, twin or mutations), bit for bit — on a case with rejections and on one with a clamp; resets = rejected pairs + dropped directions."""
    from oracle import oracle as O
    from tests import controller_ref as R
    for name, n in (("reject_midrun", 96), ("lower_clamp", 96)):
        case = T.CASES[name]
        _, _, om, of = T.models(case, n)
        d10 = R.problem(n)[1]
        force = lambda u: O.energy_force(om, d10, u, *case.weights)[0]
        x = T.start(name, n, 0).astype(np.float64).reshape(-1)
        S, Y, gamma, resets = [], [], T.first_length(case, n), 0
        for k in range(case.nlb):
            F = np.asarray(force(x.reshape(-1, 3)), dtype=np.float64).reshape(-1)
            if k > 0:
                y = F_prev - F
                sy, yy, ss = s_prev @ y, y @ y, s_prev @ s_prev
                if sy > 1e-12 * np.sqrt(ss * yy):
                    S.append(s_prev); Y.append(y)
                    if len(S) > case.mem:
                        S.pop(0); Y.pop(0)
                    gamma = sy / yy
                else:
                    S, Y, resets, gamma = [], [], resets + 1, gamma * 2.0
                gamma = min(max(gamma, 1e-7), 1e2)
            d = L.compact_direction(F, S, Y, gamma)
            if not (F @ d > 0):
                S, Y, resets, d = [], [], resets + 1, gamma * F
            step = d.reshape(-1, 3)
            ln = np.sqrt((step ** 2).sum(axis=1))
            step = step * np.where(ln > float(of.max_step), float(of.max_step) / np.maximum(ln, 1e-300), 1.0)[:, None]
            xn = x + step.reshape(-1)
            F_prev, s_prev, x = F, xn - x, xn
        xr, info = L.lbfgs_run(force, T.start(name, n, 0).astype(np.float64), case.nlb, m=case.mem, g0=T.first_length(case, n),
                               max_step=float(of.max_step))
        assert np.array_equal(xr.reshape(-1), x), name
        log = info["log"]
        assert info["resets"] == resets == sum(s.branch.count("rejected") + s.branch.count("dropped") for s in log), name
        assert len(log) == case.nlb and log[0].branch == "first" and log[0].slot == case.mem - 1


def test_cases_take_every_branch(built):
    """The table's coverage, and what the admission prints per case: branches taken and the smallest margins."""
    logs = _logs()
    for name, n, slot, log in logs:
        b = T.branches(log)
        margins = [abs(s.margin) for s in log if s.margin is not None]
        clampd = [abs(np.log(s.graw / e)) for s in log[1:] for e in (1e-7, 1e2)]
        print(f"CASE {name} n={n} slot {slot} mem {T.CASES[name].mem}: " + " ".join(
            {"first": "F", "kept": "k", "rejected": "R"}[x.split("+")[0]] + ("l" if x.endswith("+lo") else "h" if x.endswith("+hi") else "")
            for x in b) + f" | capped {[s.ncap for s in log]} | pair margin {min(margins):.3g} cosine {min(s.cos for s in log):.3g}"
            f" |ln(gamma/bound)| {min(clampd):.3g} resets {T.reference(name, n, slot)[2]}")
    seen = set()
    for name, n, slot, log in logs:
        mem = T.CASES[name].mem
        for k, s in enumerate(log):
            if s.branch == "rejected":
                after = log[k + 1:k + 4]
                if len(after) == 3 and all(t.branch == "kept" for t in after) and s.slot != 0 and [t.pairs for t in after] == [1, 2, 3][:mem] + [mem] * max(0, 3 - mem):
                    seen.add("refill, head not at slot 0")
                    if log[k - 1].pairs >= 2:
                        seen.add("refill in mid-run")
                if k + 1 < len(log) and log[k + 1].branch == "rejected":
                    seen.add("two rejections in a row")
                if k + 1 in T.CASES[name].checkpoints:
                    seen.add("split directly after a rejection")
        for side in ("lo", "hi"):
            if any(s.clamp == side for s in log) and sum(1 for s in log[1:] if s.clamp is None) >= 3:
                seen.add(side + " clamp with unclamped steps")
        if any(s.ncap == 0 for s in log[1:]):
            seen.add("no bead capped")
        if any(0 < s.ncap < n for s in log):
            seen.add("some beads capped")
        if sum(1 for s in log if s.ncap == n) >= 3:
            seen.add("all beads capped")
        full = next((k for k, s in enumerate(log) if s.pairs == mem), None)
        if full is not None and len(log) - 1 - full >= mem + 3 and all(s.branch == "kept" and s.pairs == mem for s in log[full:]):
            slots = [s.slot for s in log[full:]]
            assert all((a + 1) % mem == b_ for a, b_ in zip(slots, slots[1:])), (name, slots)
            seen.add(f"wrap-around at memory {mem}")
        if T.CASES[name].nsteps > T.CASES[name].nlb:
            seen.add("hand-over to FIRE")
    want = {"refill, head not at slot 0", "refill in mid-run", "two rejections in a row", "split directly after a rejection",
            "lo clamp with unclamped steps", "hi clamp with unclamped steps", "no bead capped", "some beads capped", "all beads capped",
            "hand-over to FIRE"} | {f"wrap-around at memory {m}" for m in (1, 2, 5, 8)}
    assert want <= seen, sorted(want - seen)
    # the stat the device test compares: resets differ between the slots of a case somewhere (a sum over replicas, not one replica's)
    assert any(T.reference(name, n, 0)[2] != T.reference(name, n, 1)[2] for name, n in T.CASE_SIZES)


@pytest.mark.parametrize("name,n", T.CASE_SIZES)
def test_float32_can_follow_the_case(built, name, n):
    """Conditioning: the float32 twin takes the restatement's branch on every step and ends every checkpoint within a quarter of the
    fp32 bound.  Margins: every pair test |s.y / sqrt(s.s y.y)| >= 1e-3, every descent cosine >= 1e-3, every gamma at least 1 % beyond the
    clamp it meets or inside the ones it does not."""
    case = T.CASES[name]
    for slot in (0, 1):
        ref, twin = T.reference(name, n, slot), T.reference(name, n, slot, round32=True)
        assert T.branches(ref[1]) == T.branches(twin[1]) and ref[2] == twin[2], (slot, T.branches(ref[1]), T.branches(twin[1]))
        assert [(s.pairs, s.slot) for s in ref[1]] == [(s.pairs, s.slot) for s in twin[1]]
        g = T.gap(ref, twin, case)
        print(f"TWIN {name} n={n} slot {slot}: {g:.2e} A")
        assert g <= 0.25 * T.CAP32, (slot, g)
        for s in ref[1]:
            assert s.margin is None or abs(s.margin) >= 1e-3, (slot, s.it, s.margin)
            assert s.cos >= 1e-3, (slot, s.it, s.cos)
            if s.it > 0:
                assert s.graw <= 0.99e-7 or s.graw >= 1.01e-7, (slot, s.it, s.graw)
                assert s.graw <= 0.99e2 or s.graw >= 1.01e2, (slot, s.it, s.graw)


@pytest.mark.parametrize("mut", sorted(L.MUTATIONS))
def test_a_mutated_restatement_ends_far_away(built, mut):
    """Sensitivity: each mutation ends at least ten fp32 bounds from the restatement at some checkpoint of some case."""
    best, where = 0.0, None
    for name, n in T.CASE_SIZES:
        if n > 250:
            continue
        for slot in (0, 1):
            g = T.gap(T.reference(name, n, slot), T.reference(name, n, slot, mut=mut), T.CASES[name])
            if g > best:
                best, where = g, (name, n, slot)
    print(f"MUTATION {mut} ({L.MUTATIONS[mut]}): {best:.3g} A at {where}")
    assert best >= 10.0 * T.CAP32, (mut, best, where)


@pytest.mark.parametrize("mem,cnt,head", [(1, 1, 0), (3, 2, 0), (5, 5, 1), (8, 8, 7), (8, 3, 1), (4, 0, 2)])
def test_table_restatement_is_the_compact_direction(mem, cnt, head):
    """lbfgs_ref.direction_row_ref — what tests/test_gpu_lbfgs_direction.py expects of c3d_debug_lbfgs_direction — on sums and a state
    formed from real vectors: after a kept pair its coefficients give compact_direction's d = gamma F + sum a_j s_j + sum b_j y_j for the
    pairs then held, in age order, whatever slots of the ring they sit in; after a rejected pair d = 2 gamma_in F and nothing is held."""
    rng = np.random.default_rng(100 * mem + 10 * cnt + head)
    n, M = 60, L.MAX_PAIRS
    s_vec = rng.normal(size=(M, n))
    y_vec = 0.7 * s_vec + 0.2 * rng.normal(size=(M, n))           # s.y > 0: curvature pairs
    F = rng.normal(size=n)
    nx = (head + 1) % mem
    for kept in (True, False):
        y_new = y_vec[nx] if kept else -y_vec[nx]
        sums = np.zeros(L.NSUMS)
        for j in range(M):
            yj = y_new if j == nx else y_vec[j]
            sums[4 * j:4 * j + 4] = F @ s_vec[j], F @ yj, s_vec[j] @ y_new, yj @ y_new
        sums[L.NSUMS - 4], sums[L.NSUMS - 3] = s_vec[nx] @ s_vec[nx], F @ F
        SY, YY = s_vec @ y_vec.T + 7.0, y_vec @ y_vec.T - 3.0       # every entry off by a constant ...
        old = [(head - (cnt - 1) + i) % mem for i in range(cnt)]    # ... but those of the pairs held before the step, oldest first
        for a, i in enumerate(old):
            for j in old[a:]:
                SY[i, j] = s_vec[i] @ y_vec[j]
            for j in old:
                YY[i, j] = y_vec[i] @ y_vec[j]
        sd = np.concatenate([[0.01], SY.reshape(-1), YY.reshape(-1)])
        si, sdo, coef, mask, slot, fd = L.direction_row_ref(sums, (cnt, head, mem, 0), sd, 0, mem, 1.0)
        if kept:
            k = min(cnt + 1, mem)
            held = [(nx - (k - 1) + i) % mem for i in range(k)]
            gamma = (s_vec[nx] @ y_new) / (y_new @ y_new)
            want = L.compact_direction(F, [s_vec[j] for j in held], [y_new if j == nx else y_vec[j] for j in held], gamma)
            got = coef[0] * F + sum(coef[1 + j] * s_vec[j] + coef[1 + M + j] * (y_new if j == nx else y_vec[j]) for j in held)
            assert si == (k, nx, mem, 0) and mask == sum(1 << j for j in held) and slot == (nx + 1) % mem and fd > 0
            assert abs(coef[0] - gamma) <= 1e-15 * gamma and np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
        else:
            assert si == (0, head, mem, 1) and mask == 0 and slot == nx and coef[0] == 0.02 and not coef[1:].any()
