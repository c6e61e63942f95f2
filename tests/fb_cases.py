"""The cases of the forward-backward tests (tests/test_fb_host.py on the CPU, tests/test_gpu_fb*.py on the GPU) and the
reference for ACCURACY: forward-backward in float64 numpy, with numpy's logaddexp (fdnn_fb.hpp states the fp32 recursion):

    alpha[0] = start + e[0];  alpha[t][j] = logsumexp over j's arcs of alpha[t-1][src] + lp, + e[t][j]
    total    = logsumexp_j alpha[T-1][j] + final[j]
    bb[T-1]  = final + e[T-1];  bb[t][i] = logsumexp over i's outgoing arcs of bb[t+1][dst] + lp, + e[t][i]
    gamma    = exp(alpha + bb - e - total)

The reference for BYTES is the C restatement (api.fb_ref); the library is never checked against itself.  Graphs are the
alignment graphs' dicts (tests/align_graph_cases.py); everything is seeded."""
import numpy as np

import align_graph_cases as GC
from fast_dnn_amd import api

U = 2.0 ** -24
K_EXP_MAX_ULP = 1.05        # fdnn_fb.hpp: kExpMaxUlp (profiles/exp_sweep.log)
K_LSE1_MAX_ABS = 1.50 * U   # fdnn_fb.hpp: kLse1MaxAbs


def ends(g):
    S = len(g["states"])
    start = np.full(S, -np.inf)
    final = np.full(S, -np.inf)
    start[0], final[S - 1] = 0.0, 0.0
    if g.get("start_lp") is not None:
        start = np.asarray(g["start_lp"], np.float64)
    if g.get("final_lp") is not None:
        final = np.asarray(g["final_lp"], np.float64)
    return start, final


def fb64(e, g):
    """e [T][S] emissions (no NaN), g a graph -> dict(total, gamma [T][S], best: the float64 best-path total, max_abs: the
    header's M, in_deg, out_deg)."""
    e = np.asarray(e, np.float64)
    T, S = e.shape
    ptr, src, lp = np.asarray(g["arc_ptr"]), np.asarray(g["arc_src"]), np.asarray(g["arc_lp"], np.float64)
    dst = np.repeat(np.arange(S), np.diff(ptr))
    start, final = ends(g)

    def sweep(first, frm, to, frames, best=False):
        d = np.empty((T, S))
        with np.errstate(all="ignore"):
            d[frames[0]] = first + e[frames[0]]
            for prev, t in zip(frames[:-1], frames[1:]):
                acc = np.full(S, -np.inf)
                cand = d[prev][frm] + lp
                if best:
                    np.maximum.at(acc, to, cand)
                else:
                    np.logaddexp.at(acc, to, cand)
                d[t] = acc + e[t]
        return d

    fwd = list(range(T))
    alpha = sweep(start, src, dst, fwd)
    bb = sweep(final, dst, src, fwd[::-1])
    vit = sweep(start, src, dst, fwd, best=True)
    with np.errstate(all="ignore"):
        total = np.logaddexp.reduce(alpha[T - 1] + final)
        best = np.max(vit[T - 1] + final)
        gamma = np.exp(alpha + bb - e - total) if np.isfinite(total) else np.zeros((T, S))
    gamma = np.where(np.isnan(gamma), 0.0, gamma)
    fin = np.concatenate([alpha[np.isfinite(alpha)], bb[np.isfinite(bb)], [0.0]])
    step = max(float(np.abs(lp).max()) if lp.size else 0.0, float(np.abs(final[np.isfinite(final)]).max()))
    max_abs = float(np.abs(fin).max()) + step  # the header's M: bounds every alpha, bb, candidate and term of the total
    return dict(total=total, gamma=gamma, best=best, max_abs=max_abs, in_deg=int(np.diff(ptr).max()) if S else 0,
                out_deg=int(np.bincount(src, minlength=S).max()) if src.size else 0)


def delta_bound(T, S, degree, max_abs):
    """fdnn_fb.hpp: delta_bound -- the derived bound on |total - total64| and on the error of alpha + bb."""
    L = U * max_abs + K_LSE1_MAX_ABS + 0.37 * U
    return T * (2 * U * max_abs + max(degree - 1, 0) * L) + U * max_abs + (8 + (S - 1) // 256) * L


def gamma_bound(delta, max_abs):
    """fdnn_fb.hpp: gamma_bound."""
    return np.exp(2 * delta + 6 * U * max_abs) * (1.0 + K_EXP_MAX_ULP * 2 * U) - 1.0 + 1.2e-38


def ref_one(rows, col, g, want_gamma=True, **kw):
    """api.fb_ref of ONE segment whose rows are a [T][ld] array -> (total float32 scalar array [1], gamma [T][S] or None)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    total, gamma = api.fb_ref(rows, [rows.shape[0]], [0], [rows.shape[1]], api.pack_graphs([g]), col, want_gamma=want_gamma, **kw)
    return total, None if gamma is None else gamma.reshape(rows.shape[0], len(g["states"]))


def soft_silence_case(seed, scale=0.5, **kw):
    """GC.silence_case with its scores scaled towards each other (3 N(0, 1) - 5 leaves one path with nearly all the mass): the
    occupancies are then soft, which is what keeps a best-path kernel from passing the occupancy tests."""
    rows, g, col = GC.silence_case(seed, **kw)
    return (rows * np.float32(scale)).astype(np.float32), g, col


def held(got_total, got_gamma, e, g):
    """The derived bound on a result against float64 -> (total error, its bound, gamma error, its bound)."""
    w = fb64(e, g)
    T, S = e.shape
    delta = delta_bound(T, S, max(w["in_deg"], w["out_deg"]), w["max_abs"])
    te = abs(float(got_total) - w["total"]) if np.isfinite(w["total"]) else (0.0 if float(got_total) == w["total"] else np.inf)
    ge = float(np.abs(np.asarray(got_gamma, np.float64) - w["gamma"]).max()) if got_gamma is not None else 0.0
    return te, delta, ge, gamma_bound(delta, w["max_abs"])
