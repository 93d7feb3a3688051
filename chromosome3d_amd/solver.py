"""Thin object view of a libc3d context (one per GPU / process)."""
import ctypes as C

import numpy as np

from . import lib as _l


def default_model(**kw):
    m = _l.Model()
    _l.load().c3d_default_model(C.byref(m))
    for k, v in kw.items():
        if not hasattr(m, k):
            raise AttributeError(f"c3d_model has no field {k}")
        setattr(m, k, v)
    return m


def default_fire(**kw):
    f = _l.FireParams()
    _l.load().c3d_default_fire(C.byref(f))
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def default_schedule(min_steps=3000, final_kind=5):
    """The library's default schedule; final_kind 8 makes its final stage an L-BFGS stage (then FIRE) instead of kind 5."""
    if final_kind not in (2, 5, 8):
        raise ValueError("final_kind is 2 (FIRE), 5 (two-point step sizes) or 8 (L-BFGS)")
    L = _l.load()
    n = L.c3d_default_schedule(None, 0, min_steps)
    arr = (_l.Stage * n)()
    L.c3d_default_schedule(arr, n, min_steps)
    arr[n - 1].kind = final_kind
    return arr


def make_stages(rows):
    arr = (_l.Stage * len(rows))()
    for k, r in enumerate(rows):
        arr[k] = _l.Stage(*r)
    return arr


class Solver:
    """c3d_ctx wrapper.  Raises lib.C3DError when no gfx950 device / library is available.

    Matrices of up to 5120 beads are accepted by default; set_option("max_beads", n) before set_if_matrix / set_restraints raises the
    limit up to 16384 (the per-step kernels then run in their chunked form).  That is consent to the memory: about 8 n npad bytes stay
    resident per context (2.1 GB at 16384) and K1 takes 21 n^2 bytes more while it runs.  precision 64 takes 2560 beads by default;
    set_option("f64_max_beads", n) before init_replicas raises that up to 16384 (8 n^2 bytes more for the fp64 target matrix).
    embed() takes up to 4549 beads by default; set_option("embed_max_beads", n) raises that up to 16384 (the eigen stage then runs tiled
    over the device; 8 n^2 bytes for the bounds + 4 n^2 per replica of a batch while it runs).  embed_form 1 / embed_batch k are test
    knobs (same bits); stat("embed_form") / stat("embed_batches") say what the last embed() ran.
    score() beyond 5120 beads ranks the IF matrix on the device: 8 n^2 bytes for the matrix and ranks plus 8 bytes per sort slot
    (3 GiB at 16384) in the context's scoring scratch."""

    def __init__(self, device=0):
        self._L = _l.load()
        self._h = C.c_void_p()
        _l.check(self._L.c3d_create(device, C.byref(self._h)))
        self.device = device
        self.n = 0
        self.nrep = 0
        self._b0 = None      # the bond length of the model last set (None: the library's default model)

    def close(self):
        if self._h:
            self._L.c3d_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- problem ----
    def set_model(self, model):
        _l.check(self._L.c3d_set_model(self._h, C.byref(model)))
        self._b0 = float(model.b0)

    def set_schedule(self, stages, fire=None, gtol=0.0, check_every=250):
        fire = fire if fire is not None else default_fire()
        _l.check(self._L.c3d_set_schedule(self._h, stages, len(stages), C.byref(fire), gtol, check_every))

    def set_option(self, key, value):
        _l.check(self._L.c3d_set_option(self._h, key.encode(), float(value)))

    def set_if_matrix(self, IF, alpha=0.5, K=11.0):
        IF = np.ascontiguousarray(IF, dtype=np.float64)
        assert IF.ndim == 2 and IF.shape[0] == IF.shape[1]
        _l.check(self._L.c3d_set_if_matrix(self._h, _l.dptr(IF), IF.shape[0], alpha, K))
        self.n = IF.shape[0]

    def set_restraints(self, n, ri, rj, rt10):
        ri, rj, rt10 = (np.ascontiguousarray(a, dtype=np.int32) for a in (ri, rj, rt10))
        _l.check(self._L.c3d_set_restraints(self._h, n, len(ri), _l.i32ptr(ri), _l.i32ptr(rj), _l.i32ptr(rt10)))
        self.n = n

    def dist10(self):
        d = np.empty((self.n, self.n), dtype=np.int32)
        _l.check(self._L.c3d_get_dist10(self._h, _l.i32ptr(d)))
        return d

    @property
    def b0(self):
        """the bond length of the model last set (the library's default model before any set_model)"""
        return self._b0 if self._b0 is not None else float(default_model().b0)

    @property
    def num_restraints(self):
        return self._L.c3d_num_restraints(self._h)

    # ---- replicas ----
    def init_replicas(self, nrep, seed=82364, first_replica=0):
        _l.check(self._L.c3d_init_replicas(self._h, nrep, seed, first_replica))
        self.nrep = nrep

    def embed(self, iters=50):
        """A7: metric-matrix distance-geometry start for every replica (n <= 4549, or up to the option embed_max_beads)."""
        _l.check(self._L.c3d_embed_replicas(self._h, iters))

    def dg_bounds(self):
        """(U, L), n x n fp32: the smoothed distance bounds embed() draws its trial distances from (c3d_dg_smoothed_bounds)."""
        U = np.empty((self.n, self.n), dtype=np.float32)
        L = np.empty((self.n, self.n), dtype=np.float32)
        _l.check(self._L.c3d_dg_smoothed_bounds(self._h, _l.fptr(U), _l.fptr(L)))
        return U, L

    def debug_if_ranks(self, IF, rng=3):
        """(rank matrix n x n fp64, saa, m): the IF side of the Spearman coefficient as the device computes it for score()
        (c3d_debug_if_ranks; symmetric matrices only)."""
        IFc = np.ascontiguousarray(IF, dtype=np.float64)
        assert IFc.shape == (self.n, self.n)
        rank = np.empty((self.n, self.n), dtype=np.float64)
        saa, m = C.c_double(), C.c_size_t()
        _l.check(self._L.c3d_debug_if_ranks(self._h, _l.dptr(IFc), rng, _l.dptr(rank), C.byref(saa), C.byref(m)))
        return rank, saa.value, m.value

    def set_coords(self, xyz):
        xyz = _l.as_f32(xyz)
        assert xyz.shape == (self.nrep, self.n, 3)
        _l.check(self._L.c3d_set_coords(self._h, _l.fptr(xyz)))

    def coords(self):
        x = np.empty((self.nrep, self.n, 3), dtype=np.float32)
        _l.check(self._L.c3d_get_coords(self._h, _l.fptr(x)))
        return x

    def velocities(self):
        v = np.empty((self.nrep, self.n, 3), dtype=np.float32)
        _l.check(self._L.c3d_get_velocities(self._h, _l.fptr(v)))
        return v

    # the same three in doubles (precision 64): the fp64 state itself, not its float mirror
    def set_coords64(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        assert xyz.shape == (self.nrep, self.n, 3)
        _l.check(self._L.c3d_set_coords_f64(self._h, _l.dptr(xyz)))

    def coords64(self):
        x = np.empty((self.nrep, self.n, 3), dtype=np.float64)
        _l.check(self._L.c3d_get_coords_f64(self._h, _l.dptr(x)))
        return x

    def velocities64(self):
        v = np.empty((self.nrep, self.n, 3), dtype=np.float64)
        _l.check(self._L.c3d_get_velocities_f64(self._h, _l.dptr(v)))
        return v

    # ---- solve ----
    def run(self):
        _l.check(self._L.c3d_run(self._h))

    def run_steps(self, nsteps):
        done = C.c_long()
        _l.check(self._L.c3d_run_steps(self._h, nsteps, C.byref(done)))
        return done.value

    def centre(self):
        _l.check(self._L.c3d_centre(self._h))

    @property
    def schedule_length(self):
        return self._L.c3d_schedule_length(self._h)

    @property
    def steps_done(self):
        return self._L.c3d_steps_done(self._h)

    def last_timing(self):
        ms, st, la = C.c_double(), C.c_long(), C.c_long()
        _l.check(self._L.c3d_last_timing(self._h, C.byref(ms), C.byref(st), C.byref(la)))
        return ms.value, st.value, la.value

    def stat(self, key):
        v = C.c_double()
        _l.check(self._L.c3d_get_stat(self._h, key.encode(), C.byref(v)))
        return v.value

    def debug_tear16(self, iterations=200000):
        """(unit reads, torn units, reads that saw a new value) of the hand-off's 16-byte store / load pair (c3d_debug_tear16)."""
        a, b, c = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        _l.check(self._L.c3d_debug_tear16(self._h, iterations, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def debug_step_scalars(self, kind, dt, t_bath, psum, state, npos):
        """The fp32 step controller as a table (c3d_debug_step_scalars): psum [K, 4], state [K, 2] = (dt, alpha), npos [K] ->
        (scalars [K, 6] = lambda, v_cm x y z, keep, mix; state out [K, 2]; npos out [K]) under the context's model and FIRE values."""
        psum, state = _l.as_f32(psum), _l.as_f32(state)
        npos = np.ascontiguousarray(npos, dtype=np.int32)
        K = npos.shape[0]
        assert psum.shape == (K, 4) and state.shape == (K, 2)
        sc, so, no = np.empty((K, 6), dtype=np.float32), np.empty((K, 2), dtype=np.float32), np.empty(K, dtype=np.int32)
        _l.check(self._L.c3d_debug_step_scalars(self._h, int(kind), float(dt), float(t_bath), K, _l.fptr(psum), _l.fptr(state), _l.i32ptr(npos),
                                                _l.fptr(sc), _l.fptr(so), _l.i32ptr(no)))
        return sc, so, no

    def debug_step_scalars_f64(self, kind, dt, t_bath, psum, state, npos):
        """The fp64 step controller as a table (c3d_debug_step_scalars_f64, precision-64 contexts): debug_step_scalars in doubles."""
        psum, state = np.ascontiguousarray(psum, dtype=np.float64), np.ascontiguousarray(state, dtype=np.float64)
        npos = np.ascontiguousarray(npos, dtype=np.int32)
        K = npos.shape[0]
        assert psum.shape == (K, 4) and state.shape == (K, 2)
        sc, so, no = np.empty((K, 6), dtype=np.float64), np.empty((K, 2), dtype=np.float64), np.empty(K, dtype=np.int32)
        _l.check(self._L.c3d_debug_step_scalars_f64(self._h, int(kind), float(dt), float(t_bath), K, _l.dptr(psum), _l.dptr(state),
                                                    _l.i32ptr(npos), _l.dptr(sc), _l.dptr(so), _l.i32ptr(no)))
        return sc, so, no

    def debug_row_finish_f64(self, kind, dt, rows):
        """The fp64 row update as a table (c3d_debug_row_finish_f64, precision-64 contexts): rows [K, 16] = x[3], v[3], F[3], lambda,
        v_cm[3], keep, mix, state dt -> [K, 10] = new x[3], new v[3], the bead's terms of the four sums."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        K = rows.shape[0]
        assert rows.shape == (K, _l.ROW_FINISH_IN)
        out = np.empty((K, _l.ROW_FINISH_OUT), dtype=np.float64)
        _l.check(self._L.c3d_debug_row_finish_f64(self._h, int(kind), float(dt), K, _l.dptr(rows), _l.dptr(out)))
        return out

    def debug_row_finish(self, kind, dt, rows):
        """The fp32 row update as a table (c3d_debug_row_finish): debug_row_finish_f64's rows in floats, through finish_row."""
        rows = _l.as_f32(rows)
        K = rows.shape[0]
        assert rows.shape == (K, _l.ROW_FINISH_IN)
        out = np.empty((K, _l.ROW_FINISH_OUT), dtype=np.float32)
        _l.check(self._L.c3d_debug_row_finish(self._h, int(kind), float(dt), K, _l.fptr(rows), _l.fptr(out)))
        return out

    def debug_lbfgs_move_rows(self, coef, mask, slot, rows):
        """The rows of an L-BFGS move as a table (c3d_debug_lbfgs_move_rows), in the context's precision: coef [17] = (gamma, a_j, b_j by
        slot), the slot mask, the slot of s, rows [K, 54] = x[3], F[3], s_j[3] x 8, y_j[3] x 8 -> [K, 10] = new x[3], ring slot `slot`
        [3], ring slot (slot + 1) % 8 [3], move.move."""
        coef, rows = np.ascontiguousarray(coef, dtype=np.float64), np.ascontiguousarray(rows, dtype=np.float64)
        K = rows.shape[0]
        assert coef.shape == (_l.LBFGS_COEFS,) and rows.shape == (K, _l.LBFGS_MOVE_ROW_IN)
        out = np.empty((K, _l.LBFGS_MOVE_ROW_OUT), dtype=np.float64)
        _l.check(self._L.c3d_debug_lbfgs_move_rows(self._h, K, _l.dptr(coef), int(mask), int(slot), _l.dptr(rows), _l.dptr(out)))
        return out

    def debug_lbfgs_direction(self, sums, state_int, state_dbl, first, mem0):
        """The serial section of the L-BFGS move as a table (c3d_debug_lbfgs_direction), in the context's precision: sums [K, 36], state_int
        [K, 4] = (cnt, head, mem, resets), state_dbl [K, 129] = (gamma, S'Y [8, 8], Y'Y [8, 8]), first [K], mem0 [K] -> (state_int out,
        state_dbl out, coef [K, 17] = gamma, a by slot, b by slot; mask_slot [K, 2]) under the context's model and FIRE values."""
        sums, state_dbl = np.ascontiguousarray(sums, dtype=np.float64), np.ascontiguousarray(state_dbl, dtype=np.float64)
        state_int, first, mem0 = (np.ascontiguousarray(a, dtype=np.int32) for a in (state_int, first, mem0))
        K = first.shape[0]
        assert sums.shape == (K, _l.LBFGS_SUMS) and state_int.shape == (K, 4) and state_dbl.shape == (K, _l.LBFGS_STATE_DOUBLES) and mem0.shape == (K,)
        si, sd = np.empty((K, 4), dtype=np.int32), np.empty((K, _l.LBFGS_STATE_DOUBLES), dtype=np.float64)
        coef, ms = np.empty((K, _l.LBFGS_COEFS), dtype=np.float64), np.empty((K, 2), dtype=np.int32)
        _l.check(self._L.c3d_debug_lbfgs_direction(self._h, K, _l.dptr(sums), _l.i32ptr(state_int), _l.dptr(state_dbl), _l.i32ptr(first),
                                                   _l.i32ptr(mem0), _l.i32ptr(si), _l.dptr(sd), _l.dptr(coef), _l.i32ptr(ms)))
        return si, sd, coef, ms

    @property
    def step_kernel_name(self):
        return self._L.c3d_step_kernel_name(self._h).decode()

    def eval(self, w_all=1.0, w_vdw=1.0, repel_s=0.85, forces=True, energies=True):
        F = np.empty((self.nrep, self.n, 3), dtype=np.float32) if forces else None
        e = np.empty((self.nrep, 3), dtype=np.float64) if energies else None
        _l.check(self._L.c3d_eval(self._h, w_all, w_vdw, repel_s, _l.fptr(F) if forces else None,
                                  _l.dptr(e) if energies else None))
        return F, e

    def eval64(self, w_all=1.0, w_vdw=1.0, repel_s=0.85, forces=True, energies=True):
        """(F, e) in doubles from the fp64 kernels at the fp64 coordinates (c3d_eval_f64, precision 64): F has the bits of the force a
        stage with these weights integrates; changes no state of the solve."""
        F = np.empty((self.nrep, self.n, 3), dtype=np.float64) if forces else None
        e = np.empty((self.nrep, 3), dtype=np.float64) if energies else None
        _l.check(self._L.c3d_eval_f64(self._h, w_all, w_vdw, repel_s, _l.dptr(F) if forces else None,
                                      _l.dptr(e) if energies else None))
        return F, e

    def energies(self):
        e = np.empty((self.nrep, 3), dtype=np.float64)
        _l.check(self._L.c3d_get_energies(self._h, _l.dptr(e)))
        return e

    def score(self, IF=None, rng=3):
        """K6 on the device: (satisfied[M], sum_dev[M], spearman[M] or None) at the current coordinates.  Models of any extent up to
        50 000 A (stat "score_wide_runs" counts the calls that needed more than the fixed 262 A histogram).  The IF ranks come from the
        host up to 5120 beads and from the device beyond, for symmetric matrices; set_option("device_ranks", 1 / -1) makes it the device
        at every size / never (stat "device_rank_runs")."""
        sat = np.empty(self.nrep, dtype=np.int32)
        dev = np.empty(self.nrep, dtype=np.float64)
        rho = np.empty(self.nrep, dtype=np.float64) if IF is not None else None
        IFc = np.ascontiguousarray(IF, dtype=np.float64) if IF is not None else None
        _l.check(self._L.c3d_score_replicas(self._h, _l.dptr(IFc) if IF is not None else None, rng, _l.i32ptr(sat), _l.dptr(dev),
                                            _l.dptr(rho) if IF is not None else None))
        return sat, dev, rho

    def compare(self, extra=None):
        """(spearman, rmsd), K x K each: pipeline.model_similarity(model a, model b) for every ordered pair of the K = nrep + len(extra)
        models, on the device (c3d_compare_replicas).  Models 0..nrep-1 are the replicas at their current coordinates; `extra` is a
        stack [E, n, 3] (or one model [n, 3]) of further models, e.g. a bundled one.  rmsd[a][b] scales a onto b: not symmetric.
        Scratch for the call: 4 bytes per pair and model plus 8 bytes per sort slot (c3d.h).  precision 64: the replicas compared are the
        float mirror of the fp64 state, what coords() returns (the other model-set methods read the fp64 state itself)."""
        ptr, E = self._extra_models(extra)
        K = self.nrep + E
        rho = np.empty((K, K), dtype=np.float64)
        rmsd = np.empty((K, K), dtype=np.float64)
        _l.check(self._L.c3d_compare_replicas(self._h, ptr, E, _l.dptr(rho), _l.dptr(rmsd)))
        return rho, rmsd

    def debug_distance_ranks(self, replica):
        """The average ranks of one replica's n(n-1)/2 distances (pairs i<j in row order) as the device computes them for compare()
        (c3d_debug_distance_ranks)."""
        rank = np.empty(max(self.n * (self.n - 1) // 2, 1), dtype=np.float64)
        _l.check(self._L.c3d_debug_distance_ranks(self._h, int(replica), _l.dptr(rank)))
        return rank

    def _extra_models(self, extra):
        """(pointer or None, count) of `extra` as the C entries take their extra models; the pointer keeps its array alive"""
        if extra is None:
            return None, 0
        ex = np.ascontiguousarray(extra, dtype=np.float64)
        if ex.ndim == 2:
            ex = ex[None]
        assert ex.ndim == 3 and ex.shape[1:] == (self.n, 3)
        return _l.dptr(ex), ex.shape[0]

    def superpose(self, reference=0, ref_xyz=None, mirror=True, apply=False, iters=0):
        """(rmsd [nrep], mirrored [nrep], mean [n, 3], rmsf [n]): every replica fitted onto replica `reference` — or onto ref_xyz [n, 3]
        when that is given (reference is then ignored) — by the least-squares rotation after centring, on the device
        (c3d_superpose_replicas).  mirror: a replica that fits better reflected through the origin is reflected (mirrored[k] = 1).
        iters > 0: generalized Procrustes, that many rounds of fitting every replica to the mean of the fitted ones; rmsd is then against
        the final mean.  mean / rmsf: the mean of the fitted models and the per-bead spread about it.  apply: the fitted coordinates
        become the replicas' (velocities zero); otherwise nothing of the solve changes.  precision 64: the fp64 state is what is fitted."""
        ref = None
        if ref_xyz is not None:
            ref = np.ascontiguousarray(ref_xyz, dtype=np.float64)
            assert ref.shape == (self.n, 3)
            reference = -1
        flags = (_l.SUPERPOSE_MIRROR if mirror else 0) | (_l.SUPERPOSE_APPLY if apply else 0)
        rmsd = np.empty(self.nrep, dtype=np.float64)
        mirrored = np.empty(self.nrep, dtype=np.int32)
        mean = np.empty((self.n, 3), dtype=np.float64)
        rmsf = np.empty(self.n, dtype=np.float64)
        _l.check(self._L.c3d_superpose_replicas(self._h, int(reference), _l.dptr(ref) if ref is not None else None, flags, int(iters),
                                                _l.dptr(rmsd), _l.i32ptr(mirrored), _l.dptr(mean), _l.dptr(rmsf)))
        return rmsd, mirrored, mean, rmsf

    def rmsd_table(self, extra=None, mirror=True):
        """(rmsd, mirrored), K x K each: the superposition of model a onto model b for every ordered pair of the K = nrep + len(extra)
        models of compare(), on the device (c3d_rmsd_table): coordinate RMSD in Angstrom after the best rotation — and reflection, where
        that fits strictly better (mirrored[a][b] = 1).  The diagonal is exactly 0."""
        ptr, E = self._extra_models(extra)
        K = self.nrep + E
        rmsd = np.empty((K, K), dtype=np.float64)
        mirrored = np.empty((K, K), dtype=np.int32)
        _l.check(self._L.c3d_rmsd_table(self._h, ptr, E, _l.SUPERPOSE_MIRROR if mirror else 0, _l.dptr(rmsd), _l.i32ptr(mirrored)))
        return rmsd, mirrored

    def _picked(self, pick):
        if pick is None:
            return None, 0
        p = np.ascontiguousarray(pick, dtype=np.int32)
        if p.ndim != 1 or p.size == 0:
            raise ValueError("pick is a non-empty list of model indices (None: all models)")
        return p, int(p.size)

    def ensemble_map(self, extra=None, pick=None, cutoff=None, mean=True, sd=True, contact=None):
        """{"mean", "sd", "contact"} -> [n, n] float64, the maps that were asked for: per bead pair the mean distance over the ensemble,
        its population standard deviation from model to model, and the share of models in which the pair is closer than `cutoff`, on the
        device (c3d_ensemble_map).  The models are those of compare(): the replicas at their current coordinates (precision 64: the fp64
        state), then `extra` [E, n, 3].  pick: the model indices that count, in summation order, repeats allowed (None: all).  contact
        defaults to whether a cutoff was given.  The matrices are symmetric bit for bit; nothing of the solve changes."""
        contact = (cutoff is not None) if contact is None else bool(contact)
        if contact and cutoff is None:
            raise ValueError("the contact map needs a cutoff")
        xptr, E = self._extra_models(extra)
        p, n_pick = self._picked(pick)
        out = {k: np.empty((self.n, self.n), dtype=np.float64) for k, on in (("mean", mean), ("sd", sd), ("contact", contact)) if on}
        ptr = lambda k: _l.dptr(out[k]) if k in out else None
        _l.check(self._L.c3d_ensemble_map(self._h, xptr, E, _l.i32ptr(p) if p is not None else None, n_pick, 0.0 if cutoff is None else float(cutoff),
                                          ptr("mean"), ptr("sd"), ptr("contact")))
        return out

    def ensemble_score(self, IF, rng=3, extra=None, pick=None, cutoff=None):
        """(rho_mean, rho_contact or None): Spearman(IF, mean distance) and, with a cutoff, Spearman(IF, contact frequency) of the
        ensemble's maps over the ordered pairs |i-j| >= rng, ranked on the device (c3d_ensemble_score).  The maps are ensemble_map's for
        the same arguments, bit for bit.  A good ensemble has rho_mean < 0 and rho_contact > 0.  IF must be symmetric."""
        IFc = np.ascontiguousarray(IF, dtype=np.float64)
        assert IFc.shape == (self.n, self.n)
        xptr, E = self._extra_models(extra)
        p, n_pick = self._picked(pick)
        rm, rc = C.c_double(), C.c_double()
        _l.check(self._L.c3d_ensemble_score(self._h, _l.dptr(IFc), int(rng), xptr, E, _l.i32ptr(p) if p is not None else None, n_pick,
                                            0.0 if cutoff is None else float(cutoff), C.byref(rm), C.byref(rc) if cutoff is not None else None))
        return rm.value, (rc.value if cutoff is not None else None)

    def geometry(self, extra=None, cutoff=3.5, sep=1):
        """A dict of arrays over the K models of compare() — the replicas at their current coordinates (precision 64: the fp64 state), then
        `extra` [E, n, 3] — computed on the device (c3d_geometry_replicas): "clashes" [K] int64, the pairs i < j, j - i >= sep, no further
        apart than `cutoff` (sep = 1: the reference's clash_count, bonded neighbours and `<=` included); "bead_clashes" [K, n] int32, every
        bead's partners in those pairs; "nearest" [K, n], its closest partner at |i-j| >= sep (inf where it has none); "chain" [K, 6]:
        bond mean, bond sd, (i,i+2) mean, (i,i+2) sd, radius of gyration, extent.  Nothing of the solve changes."""
        xptr, E = self._extra_models(extra)
        K = self.nrep + E
        out = {"clashes": np.empty(K, dtype=np.int64), "bead_clashes": np.empty((K, self.n), dtype=np.int32),
               "nearest": np.empty((K, self.n), dtype=np.float64), "chain": np.empty((K, _l.GEOMETRY_FIELDS), dtype=np.float64)}
        _l.check(self._L.c3d_geometry_replicas(self._h, xptr, E, float(cutoff), int(sep), out["clashes"].ctypes.data_as(C.POINTER(C.c_int64)),
                                               _l.i32ptr(out["bead_clashes"]), _l.dptr(out["nearest"]), _l.dptr(out["chain"])))
        return out

    def separation_profile(self, extra=None, pick=None, cutoff=None):
        """(mean [n], sd [n], contact [n] or None), indexed by the separation s = |i-j|: mean and population sd of the distances d(i, i+s)
        over all i and the picked models, and, with a cutoff, the share of them below it — R(s) and P(s), the diagonal averages of
        ensemble_map()'s matrices for the same arguments without forming the matrices (c3d_separation_profile).  s = 0: 0, 0, 1."""
        xptr, E = self._extra_models(extra)
        p, n_pick = self._picked(pick)
        mean, sd = np.empty(self.n, dtype=np.float64), np.empty(self.n, dtype=np.float64)
        contact = np.empty(self.n, dtype=np.float64) if cutoff is not None else None
        _l.check(self._L.c3d_separation_profile(self._h, xptr, E, _l.i32ptr(p) if p is not None else None, n_pick, 0.0 if cutoff is None else float(cutoff),
                                                _l.dptr(mean), _l.dptr(sd), _l.dptr(contact) if contact is not None else None))
        return mean, sd, contact

    def stratified_score(self, IF, range=3, max_sep=0, extra=None, sums=False):
        """{"rho" [K, n], "scc" [K]} and, with sums=True, "sums" [K, n, 3] int64: IF against the "%.3f" model distance inside every genomic
        separation s = |i-j|, range <= s <= max_sep (0: n-1), for the K models of compare(), the sorting and the integer sums on the
        device (c3d_stratified_score).  rho[k, s] is the Spearman coefficient of the n - s pairs (i, i+s) of model k, NaN where a side
        is constant (and outside the strata asked for); scc[k] combines the strata with HiCRep's weights — the rank correlation with the
        distance decay taken out, negative for a good model.  sums[k, s] = (C, A, B), the exact integers rho and scc are formed from
        (include/c3d.h), from which a band-limited scc follows without another call.  IF must be symmetric; nothing of the solve changes."""
        IFc = np.ascontiguousarray(IF, dtype=np.float64)
        assert IFc.shape == (self.n, self.n)
        xptr, E = self._extra_models(extra)
        K = self.nrep + E
        out = {"rho": np.empty((K, self.n), dtype=np.float64), "scc": np.empty(K, dtype=np.float64)}
        if sums:
            out["sums"] = np.empty((K, self.n, _l.STRATUM_FIELDS), dtype=np.int64)
        _l.check(self._L.c3d_stratified_score(self._h, _l.dptr(IFc), int(range), int(max_sep), xptr, E, _l.dptr(out["rho"]), _l.dptr(out["scc"]),
                                              out["sums"].ctypes.data_as(C.POINTER(C.c_int64)) if sums else None))
        return out

    def bead_scores(self, IF, range=3, beads=None, extra=None):
        """A dict of arrays over the K models of compare() and the B beads asked for (beads: ascending indices, None: every bead), on the
        device (c3d_bead_scores): "rho" [K, B], the Spearman coefficient of row i of IF against the "%.3f" distances of bead i to every bead
        at least `range` away (NaN where a side is constant: an all-zero row of IF, a row of fewer than two partners); "sums" [K, B, 3]
        int64, the exact integers C, A, B it is formed from; "restrained" [B], the number of the bead's restraints (targets of the context,
        |i-j| >= min_sep, both sides); "satisfied" [K, B], the reference's net count of them within 0.5 A; "dev_milli" [K, B] int64, the
        summed deviation of those beyond 0.2 A in thousandths of an A.  IF None: the tallies alone.  Nothing of the solve changes."""
        xptr, E = self._extra_models(extra)
        K = self.nrep + E
        b = None if beads is None else np.ascontiguousarray(beads, dtype=np.int32)
        B = self.n if b is None else int(b.size)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        out = {"restrained": np.empty(B, dtype=np.int32), "satisfied": np.empty((K, B), dtype=np.int32), "dev_milli": np.empty((K, B), dtype=np.int64)}
        IFc = None
        if IF is not None:
            IFc = np.ascontiguousarray(IF, dtype=np.float64)
            assert IFc.shape == (self.n, self.n)
            out["rho"] = np.empty((K, B), dtype=np.float64)
            out["sums"] = np.empty((K, B, _l.BEAD_FIELDS), dtype=np.int64)
        _l.check(self._L.c3d_bead_scores(self._h, _l.dptr(IFc) if IFc is not None else None, int(range), _l.i32ptr(b) if b is not None else None,
                                         0 if b is None else B, xptr, E, _l.dptr(out["rho"]) if IFc is not None else None,
                                         i64(out["sums"]) if IFc is not None else None, _l.i32ptr(out["restrained"]), _l.i32ptr(out["satisfied"]),
                                         i64(out["dev_milli"])))
        return out

    def accessibility(self, extra=None, radius=None, probe=None, n_points=96, points=None):
        """A dict of arrays over the K models of compare() — the replicas at their current coordinates (precision 64: the fp64 state), then
        `extra` [E, n, 3] — computed on the device (c3d_accessibility): "exposed" [K, n] int32, of the P points x_i + R u_p on the sphere of
        radius R = radius + probe about bead i the number that lie strictly inside no other bead's sphere of that radius (Shrake-Rupley);
        "fraction" [K, n] = exposed / P; "area" [K, n] = 4 pi R^2 fraction, the bead's accessible area in A^2; "model_area" [K], its sum
        over a model's beads; "mean_fraction" [n], the fraction's mean over the models; "device_ms", the device time of the call's kernel.
        points: [P, 3] unit vectors, used as given (None: the Fibonacci lattice of n_points points, c3d_sphere_points).  radius and probe
        default to half the model's bond length b0 each — touching beads, and a probe of a bead's size: a convention, not a measured
        value.  Nothing of the solve changes."""
        radius = 0.5 * self.b0 if radius is None else float(radius)
        probe = 0.5 * self.b0 if probe is None else float(probe)
        u = None
        if points is not None:
            u = np.ascontiguousarray(points, dtype=np.float64)
            assert u.ndim == 2 and u.shape[1] == 3
            n_points = u.shape[0]
        xptr, E = self._extra_models(extra)
        K, P = self.nrep + E, int(n_points)
        exposed = np.empty((K, self.n), dtype=np.int32)
        ms = C.c_double()
        _l.check(self._L.c3d_accessibility(self._h, xptr, E, radius, probe, _l.dptr(u) if u is not None else None, P, _l.i32ptr(exposed), C.byref(ms)))
        fraction = exposed / float(P)
        area = 4.0 * np.pi * (radius + probe) ** 2 * fraction
        return {"exposed": exposed, "fraction": fraction, "area": area, "model_area": area.sum(axis=1), "mean_fraction": fraction.mean(axis=0),
                "device_ms": ms.value}

    def compartments(self, IF=None, extra=None, pick=None, consensus=False, min_sep=1, n_vec=1, iters=200, start=None):
        """Compartment eigenvectors on the device (c3d_compartments): the leading n_vec eigenvectors of the Pearson correlation of the rows
        of the observed/expected map, by `iters` rounds of orthogonal iteration, for Q maps in this order: IF [n, n] if given, the
        distance map of every picked model (pick: indices into the K models of compare(), None: all; precision 64: the fp64 state), and
        with consensus=True the pick list's mean distance map.  A dict: "expected" [Q, n] (the mean of every diagonal), "vectors"
        [Q, n_vec, n] (unit vectors; the sign of vector 0 is the compartment call), "share" [Q, n_vec] (the eigenvalue's share of the
        correlation's trace), "residual" [Q, n_vec] (|C v - lambda v|: how far the iteration is from converged), "maps" (the names of
        the Q maps: "IF", "model <k>", "consensus"), "device_ms", and with IF "agreement" [Q-1, n_vec, n_vec] (|Pearson r| of a map's
        vector a against IF's vector b) and "same_side" [Q-1, n_vec] (the share of beads on IF's side of zero).  start: [n_vec, n]
        start vectors (None: c3d_compartment_start's).  Nothing of the solve changes."""
        n, nv = self.n, int(n_vec)
        m = None
        if IF is not None:
            m = np.ascontiguousarray(IF, dtype=np.float64)
            assert m.shape == (n, n)
        s0 = None
        if start is not None:
            s0 = np.ascontiguousarray(start, dtype=np.float64)
            assert s0.shape == (nv, n)
        xptr, E = self._extra_models(extra)
        p, n_pick = self._picked(pick)
        Kp = n_pick if p is not None else self.nrep + E
        has_if = 1 if m is not None else 0
        Q = has_if + Kp + (1 if consensus else 0)
        rows = max(nv, 1)
        out = {"expected": np.empty((Q, n)), "vectors": np.empty((Q, rows, n)), "share": np.empty((Q, rows)), "residual": np.empty((Q, rows))}
        if has_if:
            out["agreement"] = np.empty((Q - 1, rows, rows))
            out["same_side"] = np.empty((Q - 1, rows))
        ms = C.c_double()
        ptr = lambda k: _l.dptr(out[k]) if k in out else None
        _l.check(self._L.c3d_compartments(self._h, _l.dptr(m) if has_if else None, xptr, E, _l.i32ptr(p) if p is not None else None, n_pick,
                                          _l.COMPARTMENT_CONSENSUS if consensus else 0, int(min_sep), nv, int(iters), _l.dptr(s0) if s0 is not None else None,
                                          ptr("expected"), ptr("vectors"), ptr("share"), ptr("residual"), ptr("agreement"), ptr("same_side"), C.byref(ms)))
        models = [int(k) for k in p] if p is not None else list(range(Kp))
        out["maps"] = (["IF"] if has_if else []) + ["model %d" % k for k in models] + (["consensus"] if consensus else [])
        out["device_ms"] = ms.value
        return out

    def insulation(self, IF=None, extra=None, pick=None, consensus=False, windows=(5, 10, 25), contact=None, min_strength=0.0, tol=1, stage=False):
        """Insulation profiles and domain boundaries on the device (c3d_insulation), for Q maps in this order: IF [n, n] if given, every
        picked model (pick: indices into the K models of compare(), None: all; precision 64: the fp64 state), and with consensus=True
        the pick list's mean distance map.  windows: strictly ascending half-widths w of the squares (1..128, 2w + 1 <= n).  contact: a
        cutoff in Angstrom — the model and consensus maps then count contacts (d < cutoff) in the square instead of averaging the
        distance.  A dict: "mean" [Q, W, n] (the map's mean over the w x w square that straddles the bead, NaN where the square does not
        fit), "score" [Q, W, n] (log2 of mean over the row's mean; NaN for a bead without a positive mean), "boundary" [Q, W, n] int32
        (1 at a strict minimum of IF's or a contact map's score, at a strict maximum of a distance map's), "strength" [Q, W, n] (the
        extremum's prominence, 0 elsewhere), "maps" (the names of the Q maps), "windows", "device_ms", and with IF "fit_r" [Q-1, W]
        (Pearson r of a map's score against IF's: a good distance map has r < 0, a good contact map r > 0) and "fit_counts" [Q-1, W, 4]
        int32 (boundaries of strength >= min_strength: of IF, of the map, IF's with one of the map's within tol beads, the map's with
        one of IF's).  stage=True stages a tile's distances in LDS where the largest window is <= 40 (the same bytes; for measurements).  Nothing of the solve
        changes."""
        n = self.n
        m = None
        if IF is not None:
            m = np.ascontiguousarray(IF, dtype=np.float64)
            assert m.shape == (n, n)
        w = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1)
        W = len(w)
        xptr, E = self._extra_models(extra)
        p, n_pick = self._picked(pick)
        Kp = n_pick if p is not None else self.nrep + E
        has_if = 1 if m is not None else 0
        Q = has_if + Kp + (1 if consensus else 0)
        out = {"mean": np.empty((Q, W, n)), "score": np.empty((Q, W, n)), "boundary": np.empty((Q, W, n), dtype=np.int32), "strength": np.empty((Q, W, n))}
        if has_if:
            out["fit_r"] = np.empty((Q - 1, W))
            out["fit_counts"] = np.empty((Q - 1, W, 4), dtype=np.int32)
        flags = (_l.INSULATION_CONSENSUS if consensus else 0) | (_l.INSULATION_CONTACT if contact is not None else 0) | (_l.INSULATION_STAGE if stage else 0)
        ms = C.c_double()
        _l.check(self._L.c3d_insulation(self._h, _l.dptr(m) if has_if else None, xptr, E, _l.i32ptr(p) if p is not None else None, n_pick, flags,
                                        _l.i32ptr(w), W, float(contact) if contact is not None else 0.0, float(min_strength), int(tol),
                                        _l.dptr(out["mean"]), _l.dptr(out["score"]), _l.i32ptr(out["boundary"]), _l.dptr(out["strength"]),
                                        _l.dptr(out["fit_r"]) if has_if else None, _l.i32ptr(out["fit_counts"]) if has_if else None, C.byref(ms)))
        models = [int(k) for k in p] if p is not None else list(range(Kp))
        out["maps"] = (["IF"] if has_if else []) + ["model %d" % k for k in models] + (["consensus"] if consensus else [])
        out["windows"] = [int(x) for x in w]
        out["device_ms"] = ms.value
        return out

    def loops(self, IF=None, extra=None, pick=None, consensus=False, mask=None, p=2, w=5, min_sep=None, max_sep=None, thr=(1.75, 1.75, 1.5, 1.5),
              min_obs=0.0, merge=2, corner=3, pixels=None, max_peaks=4096, want_ratio=False, models=True):
        """Loop enrichment on the device (c3d_loops), for Q maps in this order: IF [n, n] if given, every picked model's distance map
        (pick: indices into the K models of compare(), None: all; models=False: none, IF alone) and with consensus=True the pick list's
        mean distance map.  mask: [n], non-zero for an unmappable bin (balance()'s "masked").  Windows of half-width w with the inner
        p x p peak left out, over pixels (i, j) with min_sep <= j - i <= max_sep (defaults: 2w + 1 and min(n - 1, 2w + 1024)).  With IF
        the pixels whose four background ratios reach thr (donut, lower-left, horizontal, vertical) and whose value reaches min_obs are
        candidates, and the peaks are the candidates no other candidate within `merge` beats.  pixels: [L, 2] pairs to score in every
        map; None: the written peaks (at most max_peaks).  A dict: "expected" [Q, S] (E of the separations "separations"), with IF
        "peaks" [written, 2] int32, "candidates", "found", "masked_pixels" and with want_ratio "ratio" [4, B, n]; with a list "pixels"
        [L, 2], "at" [Q, L, 6] (M, E, r_donut, r_ll, r_h, r_v), "closed" [Q, 2] int32 (pixels with r_donut and r_ll, of those on the loop
        side: > 1 for IF, < 1 for distances), "apa" [Q, 2w+1, 2w+1] and "p2ll" [Q]; "maps", "device_ms".  Nothing of the solve changes."""
        n = self.n
        m = None
        if IF is not None:
            m = np.ascontiguousarray(IF, dtype=np.float64)
            assert m.shape == (n, n)
        p, w = int(p), int(w)
        lo = 2 * w + 1 if min_sep is None else int(min_sep)
        hi = min(n - 1, lo + _l.LOOP_MAX_BAND - 1) if max_sep is None else int(max_sep)
        if models:
            xptr, E = self._extra_models(extra)
            pk, n_pick = self._picked(pick)
            Kp = n_pick if pk is not None else self.nrep + E
        else:
            xptr, E, pk, n_pick, Kp = None, 0, None, 0, 0
        has_if = 1 if m is not None else 0
        Q = has_if + Kp + (1 if consensus else 0)
        S = max(0, min(hi + 2 * w, n - 1) - (lo - 2 * w) + 1)
        B = max(0, hi - lo + 1)
        side = 2 * max(w, 0) + 1
        mk = np.ascontiguousarray(mask, dtype=np.int32).reshape(-1) if mask is not None else None
        assert mk is None or len(mk) == n
        t = np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)
        assert len(t) == 4
        lst = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2) if pixels is not None else None
        listed = lst is not None or has_if
        Lmax = len(lst) if lst is not None else max(int(max_peaks), 0)
        out = {"expected": np.empty((Q, S))}
        ratio = np.empty((4, B, n)) if (want_ratio and has_if) else None
        peaks = np.empty((max(int(max_peaks), 0), 2), dtype=np.int32) if has_if else None
        report = np.zeros(4, dtype=np.int32) if has_if else None
        at = np.empty((Q, Lmax, 6)) if listed else None
        closed = np.empty((Q, 2), dtype=np.int32) if listed else None
        apa = np.empty((Q, side, side)) if listed else None
        p2ll = np.empty(Q) if listed else None
        dp = lambda a: _l.dptr(a) if a is not None else None
        ip = lambda a: _l.i32ptr(a) if a is not None else None
        flags = (_l.LOOP_CONSENSUS if consensus else 0) | (0 if models else _l.LOOP_IF_ONLY)
        ms = C.c_double()
        _l.check(self._L.c3d_loops(self._h, dp(m), xptr, E, ip(pk), n_pick, flags, ip(mk), p, w, lo, hi, _l.dptr(t), float(min_obs), int(merge), int(corner),
                                   ip(lst) if lst is not None and len(lst) else (ip(np.zeros(2, np.int32)) if lst is not None else None),
                                   len(lst) if lst is not None else 0, int(max_peaks), _l.dptr(out["expected"]), dp(ratio), ip(peaks), ip(report),
                                   dp(at), ip(closed), dp(apa), dp(p2ll), C.byref(ms)))
        out["separations"] = list(range(lo - 2 * w, lo - 2 * w + S))
        if has_if:
            out["candidates"], out["found"], out["masked_pixels"] = int(report[0]), int(report[1]), int(report[3])
            out["peaks"] = peaks[:int(report[2])].copy()
            if ratio is not None:
                out["ratio"] = ratio
        if listed:
            L = len(lst) if lst is not None else int(report[2])
            out["pixels"] = lst if lst is not None else out["peaks"]
            out["at"] = np.ascontiguousarray(at.reshape(-1)[:Q * L * 6].reshape(Q, L, 6))
            out["closed"], out["apa"], out["p2ll"] = closed, apa, p2ll
        names = [int(k) for k in pk] if pk is not None else list(range(Kp))
        out["maps"] = (["IF"] if has_if else []) + ["model %d" % k for k in names] + (["consensus"] if consensus else [])
        out["device_ms"] = ms.value
        return out

    def entanglement(self, extra=None, min_sep=2, max_sep=0, bounds=None, segments=True):
        """How entangled are the models, and with which handedness?  A dict of arrays over the K models of compare() — the replicas at
        their current coordinates (precision 64: the fp64 state), then `extra` [E, n, 3] — from the Gauss double integrals over the
        chain's S = n - 1 segments, on the device (c3d_entanglement): "writhe" [K] and "acn" [K] (the average crossing number), the sums
        of the pair term g and of |g| over the ordered segment pairs min_sep <= |s - t| <= max_sep (0: S - 1); with segments=True
        "seg_writhe" and "seg_acn" [K, S], every segment's share; with bounds [D + 1] (0 = bounds[0] < ... < bounds[D] = S: D domains
        of consecutive segments) "link" and "link_abs" [K, D, D]: off the diagonal the Gauss linking integral of two domains, on it a
        domain's own writhe, symmetric bit for bit; "device_ms".  A small max_sep gives the local writhe: chirality at that scale.
        Mirroring a model negates the signed outputs exactly.  Nothing of the solve changes."""
        xptr, E = self._extra_models(extra)
        K, S = self.nrep + E, self.n - 1
        out = {"writhe": np.empty(K, dtype=np.float64), "acn": np.empty(K, dtype=np.float64)}
        if segments:
            out["seg_writhe"], out["seg_acn"] = np.empty((K, S), dtype=np.float64), np.empty((K, S), dtype=np.float64)
        b, D = None, 0
        if bounds is not None:
            b = np.ascontiguousarray(bounds, dtype=np.int32).reshape(-1)
            D = len(b) - 1
            if D >= 1:
                out["link"], out["link_abs"] = np.empty((K, D, D), dtype=np.float64), np.empty((K, D, D), dtype=np.float64)
        ptr = lambda k: _l.dptr(out[k]) if k in out else None
        ms = C.c_double()
        _l.check(self._L.c3d_entanglement(self._h, xptr, E, int(min_sep), int(max_sep), _l.i32ptr(b) if b is not None else None, D, ptr("writhe"), ptr("acn"),
                                          ptr("seg_writhe"), ptr("seg_acn"), ptr("link"), ptr("link_abs"), C.byref(ms)))
        out["device_ms"] = ms.value
        return out

    def balance(self, M, method="ice", ignore_diags=2, min_nnz=10, mask=None, w0=None, tol=1e-5, max_iters=200, target=1.0, want_matrix=True,
                check_every_round=False):
        """A raw contact matrix balanced on the device (c3d_balance_matrix): M [n, n], symmetric, finite, >= 0, n up to the context's
        max_beads; it needs no targets and no replicas and changes nothing of the solve.  method: "ice" (iterative correction until the
        variance of the relative marginals is below tol, at most max_iters updates), "vc" or "sqrt-vc" (one update; no w0).
        ignore_diags: the diagonals |i-j| < ignore_diags do not count in the marginals.  Bins listed in mask (non-zero entries), bins with
        fewer than max(min_nnz, 1) non-zeros and bins left without a kept partner get weight 0.  w0: start weights [n].  A dict:
        "weights" [n], "masked" [n] int32 (0 kept, 1 mask, 2 too few non-zeros, 3 closure), "balanced" [n, n] = (w w^T) M over all
        diagonals (None with want_matrix=False), ready for set_if_matrix, "history" (the variance of every pass, T + 1 of them), "rounds"
        (T), "converged", "var", "kept" (|U|), "masked_counts" (by reason 1, 2, 3), "mean_marginal" (before the scale to target),
        "device_ms".  check_every_round=True makes the host look at the device's round record after every round (the same bytes)."""
        m = np.ascontiguousarray(M, dtype=np.float64)
        assert m.ndim == 2 and m.shape[0] == m.shape[1]
        n = m.shape[0]
        code = {"ice": _l.BALANCE_ICE, "vc": _l.BALANCE_VC, "sqrt-vc": _l.BALANCE_SQRT_VC}.get(method, method)
        mk = np.ascontiguousarray(mask, dtype=np.int32).reshape(-1) if mask is not None else None
        start = np.ascontiguousarray(w0, dtype=np.float64).reshape(-1) if w0 is not None else None
        assert (mk is None or len(mk) == n) and (start is None or len(start) == n)
        iters = int(max_iters)
        slots = iters + 1 if code == _l.BALANCE_ICE and 0 <= iters <= _l.BALANCE_MAX_ITERS else 2
        out = {"weights": np.empty(n), "masked": np.empty(n, dtype=np.int32), "balanced": np.empty((n, n)) if want_matrix else None}
        hist, rep, ms = np.full(slots, np.nan), np.empty(_l.BALANCE_REPORT), C.c_double()
        _l.check(self._L.c3d_balance_matrix(self._h, _l.dptr(m), n, int(code), _l.BALANCE_CHECK_EVERY_ROUND if check_every_round else 0, int(ignore_diags),
                                            int(min_nnz), _l.i32ptr(mk) if mk is not None else None, _l.dptr(start) if start is not None else None, float(tol),
                                            iters, float(target), _l.dptr(out["weights"]), _l.i32ptr(out["masked"]),
                                            _l.dptr(out["balanced"]) if want_matrix else None, _l.dptr(hist), _l.dptr(rep), C.byref(ms)))
        T = int(rep[0])
        out.update(history=hist[:T + 1].copy(), rounds=T, converged=bool(rep[1]), var=float(rep[2]), kept=int(rep[3]),
                   masked_counts=[int(rep[4]), int(rep[5]), int(rep[6])], mean_marginal=float(rep[7]), device_ms=ms.value)
        return out

    def map_similarity(self, maps, h=(0,), min_sep=0, max_sep=0, keep_zeros=False, want_smoothed=False):
        """Do contact maps agree?  HiCRep's stratum-adjusted correlation coefficient of every pair of maps [Q, n, n] (2 <= Q <= 16, each
        symmetric, finite, >= 0, n up to the context's max_beads), on the device (c3d_map_similarity); it needs no targets and no
        replicas and changes nothing of the solve.  h: the half-widths of the box mean, strictly ascending, each 0..20; the strata are
        the separations min_sep..max_sep (0: n - 1); pairs that are 0 in both smoothed maps are dropped unless keep_zeros.  A dict:
        "scc" [n_h, Q, Q] (symmetric, unit diagonal, NaN where no stratum counts), "rho" [n_h, P, S] (NaN for a stratum that does not
        count), "moments" [n_h, P, S, 3] (Cxy, Cxx, Cyy), "counts" [n_h, P, S, 3] int64 (N, A, B), "pairs" (the P pairs (p, q) in the
        outputs' order), "h", with want_smoothed "smoothed" [n_h, Q, S, n] (row s - min_sep: X(i, i + s), zeros behind), "device_ms"."""
        m = np.ascontiguousarray(maps, dtype=np.float64)
        assert m.ndim == 3 and m.shape[1] == m.shape[2]
        Q, n = m.shape[0], m.shape[1]
        hw = np.ascontiguousarray(h, dtype=np.int32).reshape(-1)
        hi = int(max_sep) if max_sep else n - 1
        S, P, H = max(hi - int(min_sep) + 1, 1), Q * (Q - 1) // 2, len(hw)
        out = {"scc": np.empty((H, Q, Q)), "rho": np.empty((H, P, S)), "moments": np.empty((H, P, S, 3)), "counts": np.empty((H, P, S, 3), dtype=np.int64)}
        if want_smoothed:
            out["smoothed"] = np.empty((H, Q, S, n))
        ms = C.c_double()
        _l.check(self._L.c3d_map_similarity(self._h, _l.dptr(m), Q, n, _l.i32ptr(hw), H, int(min_sep), int(max_sep), _l.MAPSIM_KEEP_ZEROS if keep_zeros else 0,
                                            _l.dptr(out["scc"]), _l.dptr(out["rho"]), _l.dptr(out["moments"]), out["counts"].ctypes.data_as(C.POINTER(C.c_int64)),
                                            _l.dptr(out["smoothed"]) if want_smoothed else None, C.byref(ms)))
        out["pairs"] = [(p, q) for p in range(Q) for q in range(p + 1, Q)]
        out["h"] = [int(x) for x in hw]
        out["device_ms"] = ms.value
        return out

    def rank(self):
        r = np.empty(self.nrep, dtype=np.int32)
        _l.check(self._L.c3d_rank(self._h, _l.i32ptr(r)))
        return r
