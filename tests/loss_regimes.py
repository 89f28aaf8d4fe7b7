"""Inputs and references for the PPO loss at the regimes and branch points the random tests do not reach.

evaluate(d, dtype)   the one torch-autograd transcription of the reference's loss on the CPU (ppo.py:221-223 advantage
                     normalisation, :240-244 and :249-257 augmented blocks, :259-269 KL, :297-315 losses, :328-348 mirror
                     loss, torch.distributions.Normal log_prob / entropy).  The float64 call is the reference, the
                     float32 call the yardstick: what plain fp32 arithmetic loses on the same inputs.
oracle(...)          the float64 call under the name and signature tests/test_gpu_symmetry.py has always used.
make_regime(...)     named input regimes with the branch-separation condition below.
exact_table(...)     rows whose expected outputs are exact in fp32: ties of torch.max, both ends of clamp's closed
                     interval, a tie whose half share meets a blocking clamp, a zero advantage.
nonfinite_cases(...) one bad value in one row of a `late` batch; the float32 call is the reference there (where fp32
                     overflows is the semantics under test).

Branch separation (a condition on the inputs, not a measurement): no row of the float64 evaluation has its ratio within
a relative 2^-10 of 1 +- clip, |V - tv| within 2^-10 of clip, or -- for a row outside the value clip -- |vl - vlc|
within 2^-10 of the larger of the two.  fp32 evaluates the ratio to ~1e-4 at worst (the log-prob sum of the tiny_sigma
regime), ten times inside that margin, so every implementation takes the float64 branches on every row and no test built
on these inputs excuses a row.  A row inside the value clip has value_clipped == V up to rounding, so vl and vlc tie up to
rounding by construction; there both sides of the max pass their gradient to V, the sum is 2 g (V - R) whichever side
wins, and the branch is not a branch.  Rows that miss the condition get new noise (delta, V, R) until none does."""

import functools
import types

import numpy as np
import torch

CLIP, CV, CE = 0.2, 1.0, 0.01
SEP = 2.0 ** -10
STAT_KEYS = ("loss", "surrogate", "value", "entropy", "kl")
STAT_FLOOR = {"loss": 1e-6, "surrogate": 1e-6, "value": 1e-6, "entropy": 1e-6, "kl": 1e-7, "symmetry": 1e-6}
STAT_RTOL = 1e-5


def apply_maps(x, maps):
    """torch form of the augmentation: cat_k sign_k * x[:, perm_k]."""
    return torch.cat([x[:, torch.as_tensor(p, device=x.device).long()] * torch.as_tensor(s, device=x.device).to(x.dtype)
                      for p, s in maps], dim=0)


def evaluate(d, dtype, *, B=None, k_ppo=1, k_mir=1, coeff=0.0, clipped=True, norm_adv=False, clip=CLIP, cv=CV, ce=CE):
    """The reference's update lines with torch autograd in `dtype` on the CPU.

    d: mu [k_mir B, A], sigma [A] or [k_mir B, A], V [k_ppo B], x [k_ppo B, A], old_logp / adv / tv / R [B] or [B, 1],
    omu / osig [B, A], maps (k_mir > 1).  d["old_logp64"], where present, is the stored log-prob the float64 call uses
    (exact_table: the same mathematical input, log-prob == stored log-prob, rounded to each precision)."""
    def leaf(k):
        return d[k].detach().to(dtype).clone().requires_grad_()

    def const(k, width=1):
        return d[k].detach().to(dtype).reshape(-1, width)

    mu, sigma, V = leaf("mu"), leaf("sigma"), leaf("V")
    V2 = V.reshape(-1, 1)
    A = mu.shape[1]
    x, omu, osig = (const(k, A) for k in ("x", "omu", "osig"))
    adv, tv, R = (const(k) for k in ("adv", "tv", "R"))
    old_logp = const("old_logp64" if dtype == torch.float64 and "old_logp64" in d else "old_logp")
    if B is None:
        B = old_logp.shape[0]
    n = k_ppo * B
    if norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    old_logp, adv, tv, R = (t.repeat(k_ppo, 1) for t in (old_logp, adv, tv, R))
    sig_rows = sigma.expand(mu.shape[0], A) if sigma.dim() == 1 else sigma
    dist = torch.distributions.Normal(mu[:n], sig_rows[:n], validate_args=False)
    logp = dist.log_prob(x).sum(-1)
    mu_b, sig_b = mu[:B], sig_rows[:B]
    entropy = dist.entropy().sum(-1)[:B]
    with torch.no_grad():
        kl = torch.sum(torch.log(sig_b / osig + 1.0e-5) + (torch.square(osig) + torch.square(omu - mu_b))
                       / (2.0 * torch.square(sig_b)) - 0.5, dim=-1).mean()
    ratio = torch.exp(logp - old_logp.squeeze(-1))
    surrogate = -adv.squeeze(-1) * ratio
    surrogate_clipped = -adv.squeeze(-1) * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
    value_clipped = tv + (V2 - tv).clamp(-clip, clip)
    vl, vlc = (V2 - R).pow(2), (value_clipped - R).pow(2)
    if clipped:
        value_loss = torch.max(vl, vlc).mean()
    else:
        value_loss = (R - V2).pow(2).mean()
    loss = surrogate_loss + cv * value_loss - ce * entropy.mean()
    sym = torch.zeros((), dtype=dtype)
    if k_mir > 1:
        target = apply_maps(mu[:B], d["maps"]).detach()
        sym = torch.nn.functional.mse_loss(mu[B:], target[B:])
        loss = loss + coeff * sym
    loss.backward()
    with torch.no_grad():
        dv = (V2 - tv).squeeze(-1)
        out = {"dmu": mu.grad, "dsigma": sigma.grad, "dV": V.grad, "loss": loss.item(),
               "surrogate": surrogate_loss.item(), "value": value_loss.item(), "entropy": entropy.mean().item(),
               "kl": kl.item(), "symmetry": sym.item(), "ratio": ratio.detach(), "dv": dv,
               "vl": vl.detach().squeeze(-1), "vlc": vlc.detach().squeeze(-1),
               "outside_ratio": ((ratio < 1.0 - clip) | (ratio > 1.0 + clip)).double().mean().item(),
               "outside_value": (dv.abs() > clip).double().mean().item()}
    return out


def oracle(d, B, k_ppo, k_mir, coeff, clipped, norm_adv):
    """The float64 reference of the symmetric loss (tests/test_gpu_symmetry.py)."""
    return evaluate(d, torch.float64, B=B, k_ppo=k_ppo, k_mir=k_mir, coeff=coeff, clipped=clipped, norm_adv=norm_adv)


def branch_masks(r, clip=CLIP):
    """The four branches of one evaluation, per row: ratio below / above the clip range, value difference outside the
    value clip, and -- meaningful on those rows only (module docstring) -- the unclipped value loss the larger."""
    out = r["dv"].abs() > clip
    return {"ratio_lo": r["ratio"] < 1.0 - clip, "ratio_hi": r["ratio"] > 1.0 + clip, "value_out": out,
            "vl_gt": (r["vl"] > r["vlc"]) & out}


def unseparated_rows(r, clip=CLIP):
    """Rows of a float64 evaluation that miss the branch-separation condition."""
    ratio, dv, vl, vlc = r["ratio"], r["dv"], r["vl"], r["vlc"]
    bad = ((ratio - (1.0 - clip)).abs() <= SEP * (1.0 - clip)) | ((ratio - (1.0 + clip)).abs() <= SEP * (1.0 + clip))
    bad |= (dv.abs() - clip).abs() <= SEP
    bad |= (dv.abs() > clip) & ((vl - vlc).abs() <= SEP * torch.maximum(vl, vlc))
    return bad


# name: (sigma range, delta scale, value scale, advantage offset).  Beside a regime: the largest error of the float32
# yardstick on a statistic, relative to the float64 value, over the shapes the GPU test runs (B = 333; A = 4, 7, 12, 16,
# 33; shared and per-row sigma), where it misses the suite's 1e-5 |ref| + floor.  For that regime and statistic the bound
# is three times the yardstick's error on the same inputs (stat_bound, WIDENED_STATS); every other statistic of every
# regime keeps the suite's bound.  Measured on the CPU: tests/test_loss_regimes_host.py::test_print_yardstick_statistics prints the table.
REGIMES = {
    "late": ((0.03, 0.1), 0.3, 1.0, 0.0),
    "tiny_sigma": ((1e-3, 2e-3), 0.3, 1.0, 0.0),
    "wide_sigma": ((5.0, 20.0), 0.3, 1.0, 0.0),
    "saturated": ((0.5, 1.5), 3.0, 1.0, 0.0),
    "big_values": ((0.5, 1.5), 0.3, 1e3, 0.0),
    "kl_near_zero": ((0.5, 1.5), 0.3, 1.0, 0.0),  # kl: 1.6e-3 (a KL of ~5e-7 out of terms of 0.5)
    "shifted_adv": ((0.5, 1.5), 0.3, 1.0, 1e3),  # surrogate: 2.7e-3, loss: 1.3e-4 (fp32 mean / std of 1e3 + N)
}


def _logp64(mu, sigma, x):
    s = np.broadcast_to(sigma, mu.shape).astype(np.float64)
    dlt = x.astype(np.float64) - mu.astype(np.float64)
    return (-(dlt * dlt) / (2.0 * s * s) - np.log(s) - 0.5 * np.log(2.0 * np.pi)).sum(-1)


def make_regime(name, B, A, shared, seed, *, k_ppo=1, k_mir=1, clipped=True):
    """Inputs of the named regime that meet the branch-separation condition: (d, kw, masks, reference).

    d as evaluate() takes it (float32 tensors); kw: the evaluate() / kernel options the regime implies; masks: the
    branches of the float64 evaluation; reference: that evaluation.  With k_mir > 1 the augmented blocks follow
    tests/test_gpu_symmetry.py's make_inputs: means near the mapped base means, actions at the base row's deviation."""
    (s_lo, s_hi), delta_scale, v_scale, adv_off = REGIMES[name]
    rng = np.random.default_rng(seed)
    rows, n = k_mir * B, k_ppo * B
    f = np.float32
    sigma = rng.uniform(s_lo, s_hi, A if shared else (B, A)).astype(f)
    if not shared:
        sigma = np.tile(sigma, (k_mir, 1))
    sig_b = np.broadcast_to(sigma, (rows, A))[:B]
    mu = rng.standard_normal((rows, A)).astype(f)
    x = np.empty((n, A), f)
    x[:B] = (mu[:B] + sig_b * rng.standard_normal((B, A))).astype(f)
    maps = [(np.arange(A), np.ones(A, f))]
    for _ in range(k_mir - 1):
        maps.append((rng.permutation(A), rng.choice(np.array([-1.0, 1.0], f), A)))
    for k in range(1, k_mir):
        perm, sign = maps[k]
        blk = slice(k * B, (k + 1) * B)
        mu[blk] = (mu[:B][:, perm] * sign + 0.3 * sig_b * rng.standard_normal((B, A))).astype(f)
        if k < k_ppo:
            x[blk] = (mu[blk] + (x[:B] - mu[:B]) + 0.05 * sig_b * rng.standard_normal((B, A))).astype(f)
    if name == "kl_near_zero":
        osig = sig_b.copy()
        omu = (mu[:B] + 1e-3 * sig_b * rng.standard_normal((B, A))).astype(f)
    else:  # one stored sigma per action, as a rollout with a shared std parameter writes it
        osig = np.broadcast_to((sig_b[0] * rng.uniform(0.9, 1.1, A)).astype(f), (B, A)).copy()
        omu = (mu[:B] + 0.1 * sig_b * rng.standard_normal((B, A))).astype(f)
    logp = _logp64(mu[:B], sig_b, x[:B])
    adv = (adv_off + rng.standard_normal(B)).astype(f)
    tv = (v_scale * rng.standard_normal(B)).astype(f)
    kw = dict(B=B, k_ppo=k_ppo, k_mir=k_mir, clipped=clipped, norm_adv=name == "shifted_adv")
    d = {"mu": mu, "sigma": sigma, "x": x, "omu": omu, "osig": osig, "adv": adv, "tv": tv,
         "old_logp": np.empty(B, f), "V": np.empty(n, f), "R": np.empty(B, f)}
    todo = np.ones(B, bool)
    for _ in range(200):
        m = int(todo.sum())
        d["old_logp"][todo] = (logp[todo] - delta_scale * rng.standard_normal(m)).astype(f)
        d["R"][todo] = (tv[todo] + rng.standard_normal(m)).astype(f)
        for k in range(k_ppo):
            d["V"][k * B:(k + 1) * B][todo] = (tv[todo] + 0.3 * rng.standard_normal(m)).astype(f)
        t = {k: torch.from_numpy(v) for k, v in d.items()}
        t["maps"] = maps
        ref = evaluate(t, torch.float64, **kw)
        todo = unseparated_rows(ref).reshape(k_ppo, B).any(0).numpy()
        if not todo.any():
            return t, kw, branch_masks(ref), ref
    raise AssertionError(f"regime {name}: no separated draw")


def errors(got, ref, where=None):
    """(rms, max) of got - ref in float64, over the entries `where` if given."""
    e = (got.double().reshape(ref.shape) - ref.double())
    if where is not None:
        e = e[where]
    if e.numel() == 0:
        return 0.0, 0.0
    return float(e.square().mean().sqrt()), float(e.abs().max())


YARD_ORDERS = 8


def yardstick_errors(d, kw, ref, yard, where=None):
    """torch fp32's (rms, max) error against the float64 reference for d mu, d sigma and d V.

    One fp32 evaluation is one draw of its rounding errors, and a shared d sigma has only A elements (in `saturated` a
    handful of rows carry every gradient): the ratio of two implementations' errors of the same class then exceeds 2
    in a few per cent of the cases by chance.  So the yardstick is taken over YARD_ORDERS orders of the same inputs --
    the given one and row and action permutations of it, which change nothing but the order of fp32's sums: the rms
    pooled over the orders, the max averaged over them (the expected max of one draw, not the max of eight)."""
    keys = ("dmu", "dsigma", "dV")
    sq, mx, rows, A = {k: [] for k in keys}, {k: [] for k in keys}, d["mu"].shape[0], d["mu"].shape[1]
    B, k_ppo, k_mir = kw.get("B", d["old_logp"].numel()), kw.get("k_ppo", 1), kw.get("k_mir", 1)
    rng = np.random.default_rng(rows * 31 + A)
    for order in range(YARD_ORDERS):
        if order == 0:
            y = yard
        else:
            pr, pa = torch.from_numpy(rng.permutation(B)), torch.from_numpy(rng.permutation(A))
            inv_r, inv_a = torch.argsort(pr), torch.argsort(pa)
            blocks = lambda t, k: torch.cat([t[j * B:(j + 1) * B][pr] for j in range(k)])  # noqa: E731
            unblocks = lambda t, k: torch.cat([t[j * B:(j + 1) * B][inv_r] for j in range(k)])  # noqa: E731
            e = {}
            for key, t in d.items():
                if key == "maps":
                    e[key] = [(inv_a.numpy()[p_[pa.numpy()]], s_[pa.numpy()]) for p_, s_ in t]
                elif key == "sigma" and t.dim() == 1:
                    e[key] = t[pa]
                else:
                    k = {"mu": k_mir, "sigma": k_mir, "x": k_ppo, "V": k_ppo}.get(key, 1)
                    u = blocks(t, k)
                    e[key] = u[:, pa] if u.dim() == 2 and u.shape[1] == A else u
            y = evaluate(e, torch.float32, **kw)
            y = {"dmu": unblocks(y["dmu"], k_mir)[:, inv_a], "dV": unblocks(y["dV"], k_ppo),
                 "dsigma": y["dsigma"][inv_a] if y["dsigma"].dim() == 1 else unblocks(y["dsigma"], k_mir)[:, inv_a]}
        for k in keys:
            r, m = errors(y[k], ref[k], None if where is None else where[k])
            sq[k].append(r * r)
            mx[k].append(m)
    return {k: (float(np.sqrt(np.mean(sq[k]))), float(np.mean(mx[k]))) for k in keys}


@functools.lru_cache(maxsize=None)
def regime_case(name, B, A, shared, k_ppo=1, k_mir=1):
    """make_regime with a seed of its own per case, the float64 reference, the float32 yardstick and its errors;
    computed once and shared between the tests (callers leave every tensor as it is)."""
    seed = 7919 * sorted(REGIMES).index(name) + 101 * A + 13 * B + 5 * k_mir + int(shared)
    d, kw, masks, ref = make_regime(name, B, A, shared, seed, k_ppo=k_ppo, k_mir=k_mir)
    yard = evaluate(d, torch.float32, **kw)
    return types.SimpleNamespace(name=name, d=d, kw=kw, masks=masks, ref=ref, yard=yard,
                                 yard_err=yardstick_errors(d, kw, ref, yard))


RMS_BAR, MAX_BAR = 2.0, 3.0


def within_bar(got, c, what="", where=None, yard_err=None):
    """The fp32-class bar on d mu, d sigma, d V of `got` (a dict) against case c: rms error against float64 within 2x
    of the yardstick's, max within 3x (tests/test_gpu_fused_mlp.py's, test_gpu_h3.py's and test_gpu_lstm_cell.py's bar).
    Prints and returns the ratios; the caller asserts on `ok`."""
    out, ok = {}, True
    yard_err = yard_err or c.yard_err
    for k in ("dmu", "dsigma", "dV"):
        rms, mx = errors(got[k], c.ref[k], None if where is None else where[k])
        rms32, mx32 = yard_err[k]
        out[k] = (rms / rms32 if rms32 else (np.inf if rms else 0.0), mx / mx32 if mx32 else (np.inf if mx else 0.0))
        fin = c.ref[k][torch.isfinite(c.ref[k])].abs()
        print(what, k, "rms x%.2f max x%.2f of fp32 (max err %.1e of the tensor's max)"
              % (out[k] + (mx / (float(fin.max()) + 1e-300 if fin.numel() else 1.0),)))
        ok = ok and rms <= RMS_BAR * rms32 and mx <= MAX_BAR * mx32
    return ok, out


# (regime, statistic) pairs where the float32 yardstick misses the suite's bound (the figures beside REGIMES)
WIDENED_STATS = {("kl_near_zero", "kl"), ("shifted_adv", "surrogate"), ("shifted_adv", "loss")}


def stat_bound(key, ref, yard, regime=None):
    """The suite's bound on a statistic, 1e-5 |ref| + floor.  For the (regime, statistic) pairs of WIDENED_STATS, and
    only for those: three times the float32 yardstick's error on the same inputs, where that misses the suite's bound."""
    std = STAT_RTOL * abs(ref[key]) + STAT_FLOOR[key]
    if (regime, key) not in WIDENED_STATS:
        return std
    err32 = abs(yard[key] - ref[key])
    return std if err32 <= std else 3.0 * err32


# ------------------------------------------------------------------------------------------------ exact table
_LOG_SQRT_2PI = np.float32(0.9189385)
_OFFSETS = (0.0, 0.25, -0.25, 0.5, 1.0)
_ADVS = (1.0, -1.0, 0.5, -3.0, 0.0, -0.0)
TABLE_ROWS, TABLE_REPEAT = 32, 16


def _logp_terms(dl):
    """The fp32 log-prob terms of offsets dl at sigma = 1: (-(d d) 0.5 - 0) - 0.9189385f."""
    dl = np.asarray(dl, np.float32)
    return (-(dl * dl) * np.float32(0.5) - np.float32(0.0)) - _LOG_SQRT_2PI


def _order_free(dl):
    """The sequential sum of the terms and, at 4 actions, the quad-order sum (t0 + t1) + (t2 + t3): the same bits?"""
    t = _logp_terms(dl)
    seq = np.float32(0.0)
    for v in t:
        seq = np.float32(seq + v)
    if len(t) == 4 and np.float32(np.float32(t[0] + t[1]) + np.float32(t[2] + t[3])).tobytes() != seq.tobytes():
        return None
    return seq


def exact_table(A, clip, ce, per_row_sigma=False):
    """B = 512 rows (a 32-row table, 16 times) with sigma = 1, value_loss_coef = 1 and every expected output exact in
    fp32: (d, kw).  clip: 0.25 or 0; ce: 2^-7 or 0; A: 2 (order-free) or 4 (both kernels).

    Surrogate side: x - mu per action from {0, +-0.25, 0.5, 1}, the stored log-prob the fp32 sum of the log-prob's own
    terms, so the ratio is exp(0) = 1: strictly inside the clip range at 0.25 (surr == surr_c, a tie with both sides
    passing the gradient) and on both bounds at once at 0.  Advantages from {1, -1, 0.5, -3, 0, -0}.
    Value side (u = clip, or 0.25 at clip 0): V - tv from {0, +-u, +-2u, +-u/2}; at +-2u the return sits on the target's
    side (vl > vlc: the whole gradient), beyond V (vl < vlc: the clamp blocks it, zero) and midway between V and the
    clipped value (vl == vlc: the tie's half share meets the blocking clamp, half the gradient)."""
    assert A in (2, 4) and clip in (0.25, 0.0) and ce in (2.0 ** -7, 0.0)
    f = np.float32
    patterns = []
    rng = np.random.default_rng(A)
    while len(patterns) < TABLE_ROWS:  # offsets whose sum does not depend on the order (asserted again below)
        dl = rng.choice(np.array(_OFFSETS, f), A)
        if _order_free(dl) is not None:
            patterns.append(dl)
    u = clip if clip > 0 else 0.25
    vkinds = []  # (V - tv, R - tv)
    for s in (1.0, -1.0):
        vkinds += [(2 * u * s, 0.0), (2 * u * s, 3 * u * s), (2 * u * s, (2 * u + clip) * s / 2)]  # vl >, <, == vlc
        vkinds += [(u * s, 1.0), (u * s / 2, -1.0), (u * s, u * s), (u * s / 2, 0.5)]  # on / inside the bound
    vkinds += [(0.0, 1.0), (0.0, 0.0)]
    mus = np.array([0.0, 0.5, -1.5, 2.0], f)
    tvs = np.array([0.0, 1.0, -2.0, 0.5], f)
    mu, x, adv, tv, V, R, old_logp = (np.zeros(s, f) for s in ((TABLE_ROWS, A), (TABLE_ROWS, A), TABLE_ROWS, TABLE_ROWS,
                                                                TABLE_ROWS, TABLE_ROWS, TABLE_ROWS))
    for i in range(TABLE_ROWS):
        mu[i] = mus[(i + np.arange(A)) % 4]
        x[i] = mu[i] + patterns[i]
        assert np.array_equal(x[i] - mu[i], patterns[i])
        seq = _order_free(patterns[i])
        assert seq is not None, "the fp32 log-prob sum of a table row depends on its order"
        old_logp[i] = seq
        adv[i] = _ADVS[(i + i // 6) % 6]
        dv, dr = vkinds[i % len(vkinds)]
        tv[i] = tvs[(i // len(vkinds) + i) % 4]
        V[i], R[i] = tv[i] + f(dv), tv[i] + f(dr)
        assert f(V[i] - tv[i]) == f(dv) and f(R[i] - tv[i]) == f(dr)
    rep = lambda a: np.tile(a, (TABLE_REPEAT,) + (1,) * (a.ndim - 1))  # noqa: E731
    B = TABLE_ROWS * TABLE_REPEAT
    sigma = np.ones((B, A) if per_row_sigma else A, f)
    d = {"mu": rep(mu), "sigma": sigma, "x": rep(x), "omu": rep(mu), "osig": np.ones((B, A), f), "adv": rep(adv),
         "tv": rep(tv), "V": rep(V), "R": rep(R), "old_logp": rep(old_logp)}
    d = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
    # the same input for the float64 reference: stored log-prob == log-prob, in its own precision
    d["old_logp64"] = torch.from_numpy(_logp64(d["mu"].numpy(), np.ones(A), d["x"].numpy()))
    return d, dict(clip=clip, cv=1.0, ce=ce)


def ulps(got, ref):
    """|got - ref| in units of fp32's spacing at ref."""
    return abs(float(got) - float(ref)) / float(np.spacing(np.float32(abs(ref))))


# ------------------------------------------------------------------------------------------------ non-finite table
NONFINITE_ROW = 70  # the second 64-sample tile, not its first lane
NONFINITE = ("mu_nan", "V_nan", "adv_inf", "R_inf", "ratio_overflow_adv_pos", "ratio_overflow_adv_neg",
             "ratio_overflow_adv_zero", "x_inf", "sigma_nan")


def nonfinite_case(name, A, shared):
    """A `late` batch of 333 rows with one bad value in row NONFINITE_ROW (sigma_nan: one action's sigma -- the shared
    one, or that row's): inputs, float64 evaluation, float32 evaluation (the reference of the masks), the entries
    finite in both and the yardstick's errors on them."""
    c0 = regime_case("late", 333, A, shared)
    kw = c0.kw
    d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c0.d.items()}
    r, a = NONFINITE_ROW, A // 2
    nan, inf = float("nan"), float("inf")
    if name == "mu_nan":
        d["mu"][r, a] = nan
    elif name == "V_nan":
        d["V"][r] = nan
    elif name == "adv_inf":
        d["adv"][r] = inf
    elif name == "R_inf":
        d["R"][r] = inf
    elif name.startswith("ratio_overflow"):
        d["old_logp"][r] = -200.0  # the row's log-prob is about +20 at these sigmas: exp(220) overflows fp32
        d["adv"][r] = {"pos": 1.5, "neg": -1.5, "zero": 0.0}[name.rsplit("_", 1)[1]]
    elif name == "x_inf":
        d["x"][r, a] = inf
    elif name == "sigma_nan":
        if shared:
            d["sigma"][a] = nan
        else:
            d["sigma"][r, a] = nan
    else:
        raise KeyError(name)
    ref, yard = evaluate(d, torch.float64, **kw), evaluate(d, torch.float32, **kw)
    finite = {k: torch.isfinite(yard[k]) & torch.isfinite(ref[k]) for k in ("dmu", "dsigma", "dV")}
    return types.SimpleNamespace(name="late", d=d, kw=kw, ref=ref, yard=yard, finite=finite,
                                 yard_err=yardstick_errors(d, kw, ref, yard, finite))


def same_nonfinite(got, ref):
    """NaN where ref is NaN, +inf where +inf, -inf where -inf, finite elsewhere."""
    got, ref = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    return bool(torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isposinf(got), torch.isposinf(ref))
                and torch.equal(torch.isneginf(got), torch.isneginf(ref)))
