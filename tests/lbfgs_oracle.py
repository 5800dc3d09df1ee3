"""High-precision numpy definition of what sqfa_amd/csrc/lbfgs_kernels.hip computes (sqfa_lbfgs_push, sqfa_lbfgs_direction,
sqfa_lbfgs_step_stats), with the elementwise error bound the GPU tests hold the kernels to.  Imports nothing from sqfa_amd.  Conventions (Val, unit,
rounded, C_FACTOR) are those of tests/projection_oracle.py: a result `out` of arithmetic with unit roundoff u is accepted
when, elementwise,
    |out - value| <= C_FACTOR * n * u * mag                                      (ratio() <= C_FACTOR)

Reference.  direction_reference() evaluates the textbook TWO-LOOP recursion exactly as torch.optim.LBFGS writes it (newest to
oldest, then oldest to newest, rho_i = 1 / y_i.s_i from the vectors themselves) -- deliberately not the compact form of the
kernel -- on inputs already rounded to the kernel's dtype: in float64 for a float32 kernel, in np.longdouble for a float64
kernel (LONGDOUBLE_OK: eps < 1e-18; where that does not hold the float64 accuracy cases are skipped, never judged against
float64).  sy_reference() is SY[i][j] = s_i . y_j in the same precision, n = the vector length, mag = |s_i| . |y_j|.

Bound of the direction.  The kernel evaluates, with U = triu(SY) in chronological order (its lower solve uses U^T),
    b0 = -S g        al = U^-1 b0        r0 = H (-g - Y^T al)        yr = Y r0
    c  = U^-T (diag(SY) al - yr)         d  = r0 + S^T c
Each stage commits a local rounding error of (number of terms) * u * (the stage with every term replaced by its absolute
value) [Higham, Accuracy and Stability of Numerical Algorithms, sections 3.1 and 8.1] and passes on the error of the stage
before, to first order through the absolute value of the linear map applied.  In units of u, for vectors of length n and
k pairs (e_x is the bound of x; E the elementwise error of the SY handed to the kernel, in units of u: |SY| when the
test rounds the oracle's SY to the dtype, n |S| |Y|^T when SY itself came out of length-n dot products):
    e_b0  = n |S| |g|
    e_al  = |U^-1| (e_b0 + (k + 2) |U| |al| + triu(E) |al|)       substitution with reciprocal pivots: k + 2 roundings a row
    e_r0  = (k + 3) |H| (|g| + |Y|^T |al|) + |H| |Y|^T e_al
    e_yr  = n |Y| |r0| + |Y| e_r0
    e_rhs = 2 (|diag| |al| + |yr|) + |diag| e_al + diag(E) |al| + e_yr
    e_c   = |U^-T| (e_rhs + (k + 2) |U|^T |c| + triu(E)^T |c|)
    e_d   = (k + 3) (|r0| + |S|^T |c|) + e_r0 + |S|^T e_c
|U^-1| is formed explicitly in the high precision (k <= 128).  The returned Val has n = 2 n + 4 k + 12 (the links' counts)
and mag = e_d / n, so that n u mag is the composed first-order bound; second-order terms are left to C_FACTOR = 2.  The
bound is a worst case over summation orders: at n = 30724 in float32 it allows about 1e-2 of relative error, which is why
the histories below are built so that a subtle mistake is a LARGE error (see make_history).

compact_direction() is a second evaluator: the kernel's compact form in plain numpy in a chosen dtype and summation order,
with planted mistakes as options (MISTAKES).  tests/test_lbfgs_oracle.py uses it to show that honest float32 arithmetic
stays inside the bound in two summation orders and that every planted mistake lands at least 10x outside it.
"""
import functools

import numpy as np

from projection_oracle import C_FACTOR, Val, rounded, unit  # noqa: F401  (same conventions, re-exported)

F64 = np.float64
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(LD).eps < 1e-18)
LONGDOUBLE_REASON = "np.longdouble is no wider than float64 here: no reference for the float64 kernels"
MAX_HISTORY = 128


def high_precision(dtype):
    """The precision the reference of a kernel of `dtype` is evaluated in."""
    return F64 if np.dtype(dtype) == np.dtype(np.float32) else LD


def ratio(out, val, dtype):
    """Largest |out - value| / (n u mag) over the elements, the difference taken in the precision of `value` (a float64
    result is never compared with a reference rounded to float64).  Zero magnitude: must be exact; not finite: inf."""
    hp = np.asarray(val.value).dtype
    out = np.asarray(out).astype(hp)
    value = np.asarray(val.value)
    assert out.shape == value.shape, (out.shape, value.shape)
    if not np.isfinite(out).all():
        return float("inf")
    err = np.abs(out - value).astype(F64)
    den = np.broadcast_to(np.asarray(val.n, dtype=F64) * unit(dtype) * np.asarray(val.mag, dtype=F64), err.shape)
    zero = den == 0
    if (err[zero] != 0).any():
        return float("inf")
    if zero.all():
        return 0.0
    return float((err[~zero] / den[~zero]).max())


# ---- references -----------------------------------------------------------------------------------------------------


def two_loop(S, Y, g, H, hp=F64):
    """d = -H_k g by the two-loop recursion of torch.optim.LBFGS.step: S, Y (k, n) chronological (oldest first), g (n),
    H the scalar H_diag.  Everything in `hp`."""
    S, Y, g, H = np.asarray(S).astype(hp), np.asarray(Y).astype(hp), np.asarray(g).astype(hp), hp(H)
    k = S.shape[0]
    ro = [hp(1) / np.dot(Y[i], S[i]) for i in range(k)]
    al = [None] * k
    q = -g
    for i in range(k - 1, -1, -1):
        al[i] = np.dot(S[i], q) * ro[i]
        q = q - al[i] * Y[i]
    r = q * H
    for i in range(k):
        be = np.dot(Y[i], r) * ro[i]
        r = r + S[i] * (al[i] - be)
    return r


def sy_reference(S, Y, hp=F64):
    """SY[i][j] = s_i . y_j for all rows of S and Y (any number of rows each): Val with n = the vector length."""
    S, Y = np.asarray(S), np.asarray(Y)
    value = np.dot(S.astype(hp), Y.astype(hp).T)
    return Val(value, np.abs(S.astype(F64)) @ np.abs(Y.astype(F64)).T, S.shape[1])


def upper_inverse(U):
    """Inverse of an upper triangular matrix by back substitution, in the precision of U."""
    k = U.shape[0]
    X = np.zeros_like(U)
    eye = np.eye(k, dtype=U.dtype)
    for i in range(k - 1, -1, -1):
        X[i] = (eye[i] - np.dot(U[i, i + 1:], X[i + 1:])) / U[i, i]
    return X


def direction_reference(S, Y, g, H, dtype, SY=None, sy_from="rounded"):
    """Val of the search direction for a kernel of `dtype`: value by two_loop() in high_precision(dtype), magnitude and
    term count from the stage-by-stage bound of the module docstring.  S, Y (k, n) chronological, already rounded to
    `dtype`.  SY (k, k): the matrix the code under test is given (default: the reference's, rounded to `dtype`).
    sy_from: "rounded" (SY is the high-precision product rounded once) or "dots" (SY was itself summed in `dtype`)."""
    hp = high_precision(dtype)
    assert hp is F64 or LONGDOUBLE_OK, LONGDOUBLE_REASON
    S64, Y64, g64, H64 = np.asarray(S, dtype=F64), np.asarray(Y, dtype=F64), np.asarray(g, dtype=F64), abs(float(H))
    k, n = S64.shape
    value = two_loop(S, Y, g, H, hp)
    sy = sy_reference(S, Y, hp)
    if SY is None:
        SY = sy.value.astype(dtype)
    U = np.triu(np.asarray(SY).astype(hp))
    Uinv = np.abs(upper_inverse(U)).astype(F64)
    Ua = np.abs(U).astype(F64)
    E = np.triu(Ua if sy_from == "rounded" else n * sy.mag)
    assert sy_from in ("rounded", "dots")
    # the stages in float64 (their values only weigh the bound)
    U64 = U.astype(F64)
    solve = np.linalg.solve
    b0 = -S64 @ g64
    al = solve(U64, b0)
    r0 = float(H) * (-g64 - Y64.T @ al)
    yr = Y64 @ r0
    dg = np.diag(U64)
    c = solve(U64.T, dg * al - yr)
    Sa, Ya, ga, ala, ca = np.abs(S64), np.abs(Y64), np.abs(g64), np.abs(al), np.abs(c)
    e_b0 = n * (Sa @ ga)
    e_al = Uinv @ (e_b0 + (k + 2) * (Ua @ ala) + E @ ala)
    e_r0 = (k + 3) * H64 * (ga + Ya.T @ ala) + H64 * (Ya.T @ e_al)
    e_yr = n * (Ya @ np.abs(r0)) + Ya @ e_r0
    e_rhs = 2 * (np.abs(dg) * ala + np.abs(yr)) + np.abs(dg) * e_al + np.diag(E) * ala + e_yr
    e_c = Uinv.T @ (e_rhs + (k + 2) * (Ua.T @ ca) + E.T @ ca)
    e_d = (k + 3) * (np.abs(r0) + Sa.T @ ca) + e_r0 + Sa.T @ e_c
    n_terms = 2 * n + 4 * k + 12
    return Val(value, e_d / n_terms, n_terms)


def step_stats_reference(g, g_prev, d, t, dtype):
    """sqfa_lbfgs_step_stats: y = g - g_prev and s = t d, each ONE rounded operation of `dtype` (exact to compare with), and
    Val(s) of [max|g|, max|s|, y.s, y.y, y.s / y.y] on those rounded y, s: the maxima exact (mag 0), the sums with
    n = the length, the quotient with the two relative bounds added and one more rounding."""
    hp = high_precision(dtype)
    g, g_prev, d = (np.asarray(a).astype(dtype) for a in (g, g_prev, d))
    n = g.size
    y = (g - g_prev).astype(dtype)
    s = (dtype(t) * d).astype(dtype)
    yh, sh = y.astype(hp), s.astype(hp)
    ys, yy = np.dot(yh, sh), np.dot(yh, yh)
    ys_mag = float(np.dot(np.abs(y.astype(F64)), np.abs(s.astype(F64))))
    yy_mag = float(yy)
    value = np.array([np.abs(g).max(), np.abs(s).max(), ys, yy, ys / yy], dtype=hp)
    q_mag = (ys_mag / yy_mag + abs(float(ys)) / yy_mag) if yy_mag > 0 else 0.0
    mag = np.array([0.0, 0.0, ys_mag, yy_mag, q_mag])
    return y, s, Val(value, mag, np.array([1, 1, n, n, n + 1]))


# ---- the compact form as the kernel evaluates it, with planted mistakes ----------------------------------------------

MISTAKES = ("transposed_triangle", "swapped_slots", "dropped_last_element", "dropped_first_element", "combine_tail_skipped",
            "solve_tail_skipped", "stale_row")


def mistake_reachable(mistake, n, slots, spike=None):
    """Whether the planted mistake changes the result at this shape by more than rounding.  In one dimension the newest
    pair IS H (H = s.y / y.y = s / y): dropping its terms leaves d = -H g, nothing to find.  A dropped first / last
    element is an error of order one only where that element is a spike (make_history: "head" / "tail"); elsewhere it
    changes a dot product by 1 / n of itself, far inside a worst-case bound of n u."""
    k = len(slots)
    if mistake in ("transposed_triangle", "swapped_slots"):
        return k >= 2
    if mistake == "solve_tail_skipped":
        return k % 4 != 0
    if mistake == "combine_tail_skipped":
        return k % 4 != 0 and n >= 2
    if mistake == "stale_row":
        return list(slots) != list(range(k))
    if mistake == "dropped_first_element":
        return spike == "head" and n >= 2
    if mistake == "dropped_last_element":
        return spike == "tail" and n >= 2
    raise ValueError(mistake)


def _dots(M, v, dtype, order, drop):
    """Row-wise M v in `dtype`.  order "sequential": one accumulator, index order.  order "parts": 16 chunks (a multiple
    of 4 long), 4 interleaved accumulators each, (a0 + a1) + (a2 + a3), chunks added in index order.
    drop: None, "last" (element n - 1 left out) or "first"."""
    M, v = np.asarray(M).astype(dtype), np.asarray(v).astype(dtype)
    prod = M * v[None, :]
    if drop == "last":
        prod[:, -1] = 0
    elif drop == "first":
        prod[:, 0] = 0
    rows, n = prod.shape
    if order == "sequential":
        return np.cumsum(prod, axis=1, dtype=dtype)[:, -1]
    assert order == "parts"
    chunk = ((n + 15) // 16 + 3) // 4 * 4
    pad = np.zeros((rows, 16 * chunk), dtype=dtype)
    pad[:, :n] = prod
    acc = np.cumsum(pad.reshape(rows, 16, chunk // 4, 4), axis=2, dtype=dtype)[:, :, -1, :]
    per_part = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    return np.cumsum(per_part, axis=1, dtype=dtype)[:, -1]


def _solve(Tm, x, dtype, lower, skip_last):
    """T^-1 x by column-oriented substitution with reciprocal pivots, in `dtype` (the order of lb_solve)."""
    k = len(x)
    x = np.array(x, dtype=dtype)
    rd = (dtype(1) / np.diag(Tm)).astype(dtype)
    order = range(k) if lower else range(k - 1, -1, -1)
    for step, i in enumerate(order):
        if skip_last and step == k - 1:
            break
        piv = dtype(x[i] * rd[i])
        x[i] = piv
        if lower:
            x[i + 1:] = x[i + 1:] - Tm[i + 1:, i] * piv
        else:
            x[:i] = x[:i] - Tm[:i, i] * piv
    return x


def _combine(M, coef, dtype, skip_tail):
    """sum_i coef[i] M[i] with four accumulators over the groups of four and the tail on the first one (lb_combine)."""
    k, n = M.shape
    acc = np.zeros((4, n), dtype=dtype)
    full = k - k % 4
    for i in range(full):
        acc[i % 4] = acc[i % 4] + coef[i] * M[i]
    for i in range(full, k - 1 if skip_tail else k):
        acc[0] = acc[0] + coef[i] * M[i]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def compact_direction(S_ring, Y_ring, SY_ring, slots, g, H, dtype, order="sequential", mistake=None):
    """The direction from the RING buffers (h, n), (h, n), (h, h) and the chronological `slots`, the way the kernel
    does it, every operation in `dtype`.  mistake: None or one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    h, n = np.asarray(S_ring).shape
    slots = list(slots)
    k = len(slots)
    if mistake == "swapped_slots":
        slots[-2], slots[-1] = slots[-1], slots[-2]
    rows = list(slots)
    if mistake == "stale_row":   # the newest pair is read from the row the ring index alone would give
        rows[-1] = (k - 1) if slots[-1] != k - 1 else (slots[-1] + 1) % h
    S = np.asarray(S_ring).astype(dtype)[rows]
    Y = np.asarray(Y_ring).astype(dtype)[rows]
    SYc = np.asarray(SY_ring).astype(dtype)[np.ix_(slots, slots)]
    if mistake == "transposed_triangle":
        SYc = SYc.T
    U = np.triu(SYc)
    g = np.asarray(g).astype(dtype)
    Hd = dtype(H)
    drop = {"dropped_last_element": "last", "dropped_first_element": "first"}.get(mistake)
    b0 = -_dots(S, g, dtype, order, drop)
    skip_solve = mistake == "solve_tail_skipped" and k % 4 != 0   # the last group of four is the tail
    al = _solve(U, b0, dtype, False, skip_solve)
    r0 = (Hd * (-g - _combine(Y, al, dtype, mistake == "combine_tail_skipped"))).astype(dtype)
    yr = _dots(Y, r0, dtype, order, drop)
    rhs = (np.diag(U) * al - yr).astype(dtype)
    c = _solve(U.T, rhs, dtype, True, skip_solve)
    return (r0 + _combine(S, c, dtype, mistake == "combine_tail_skipped")).astype(dtype)


# ---- seeded histories (shared by the CPU and the GPU test file) -------------------------------------------------------

SHARED = 2.0          # weight of the component w that every step shares with g
SCALE_RANGE = (0.25, 2.0)
SPIKES = ("head", "tail")
SPIKE = 2.0           # spikes are SPIKE sqrt(n) ... 1.25 SPIKE sqrt(n) large
LEAK = 2.0 ** -10     # size of a step outside its own stretch of the vector (no exact zeros anywhere)


def rng_for(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def rotated_slots(h, k, start=3):
    """k ring rows in chronological order of a ring of h rows that has wrapped: start, start + 1, ..., mod h."""
    return [(start + i) % h for i in range(k)]


def make_history(n, h, slots, dtype, spike=None, seed=0):
    """Ring buffers and a gradient for which the history MATTERS and SY is far from symmetric, rounded to `dtype`:
        s_i = m_i o (z_i + SHARED w)  (one shared w),   y_i = D_i o s_i,   g = z + w,
    D_i = a_i (1 + 0.25 U[0, 1)^n) elementwise with one scale a_i per pair, alternating between the two ends of SCALE_RANGE
    from one pair to the next (the newest at the low end), so s_i . y_i > 0.  m_i is a window: the vector is cut into k + 1 stretches and the i-th
    pair (chronological) lives on stretches i and i + 1 -- m_i = 1 there and LEAK elsewhere (m_i = 1 everywhere while
    n < 2 (k + 1)).  Neighbours in time overlap on one stretch, where s_i . y_j ~ SHARED^2 a_j x (its length) is as
    large as the diagonal and SY[i][j] / SY[j][i] ~ a_j / a_i is far from 1; pairs further apart hardly touch.
    Why windows: the bound of the module docstring is a worst case, and with k dense steps its |Y| |Y|^T |U^-1| products
    grow like k n while honest rounding errors average out -- at k = 128 the bound of a dense history exceeds |d|
    itself and no mistake could be told from rounding.  With windows every product in the bound is banded, the bound
    stays a small multiple of n u |d| elementwise, and a transposed triangle, exchanged slots, a skipped step or a
    stale row is an error of the order of d itself on the stretches of the pairs it touches.
    The ring rows outside `slots` hold dense pairs of the same kind (stale pairs, as a wrapped ring holds them).
    spike: entries of magnitude SPIKE sqrt(n) in g and in the newest s (and thereby y), "head": at index 0, "tail": at the
    last three indices (the last one from n = 4096 on: the worst-case bound of n u leaves room for one only).  The
    product of two spikes is larger than the rest of the dot product: a dropped head or tail element is an error of
    order one.
    Returns a dict: S, Y (h, n), SY (h, h; the reference's, rounded), slots, g (n), H (the newest pair's y.s / y.y)."""
    slots = list(slots)
    k = len(slots)
    assert 1 <= k <= h <= MAX_HISTORY and len(set(slots)) == k
    rng = rng_for(21, n, h, k, slots[0], ((None,) + SPIKES).index(spike or None), seed)
    w = rng.standard_normal(n)
    S = rng.standard_normal((h, n)) + SHARED * w
    if n >= 2 * (k + 1):
        edges = np.linspace(0, n, k + 2).astype(int)  # k + 1 stretches
        for i, r in enumerate(slots):
            m = np.full(n, LEAK)
            m[edges[i]:edges[i + 2]] = 1.0
            S[r] *= m
    a = np.sqrt(SCALE_RANGE[0] * SCALE_RANGE[1]) * (1.0 + 0.1 * rng.random(h))
    for i, r in enumerate(reversed(slots)):   # newest at the low end, then alternating: neighbours differ by the whole range
        a[r] = SCALE_RANGE[i % 2] * (1.0 + 0.1 * rng.random())
    D = a[:, None] * (1.0 + 0.25 * rng.random((h, n)))
    g = rng.standard_normal(n) + w
    if spike:
        assert spike in SPIKES
        idx = [0] if spike == "head" else list(range(n - (3 if n < 4096 else 1), n))
        idx = [e for e in idx if 0 <= e < n]
        amp = SPIKE * np.sqrt(n) * (1.0 + 0.25 * rng.random(len(idx)))
        g[idx] = amp * np.where(rng.random(len(idx)) < 0.5, -1.0, 1.0)
        S[slots[-1], idx] = amp
    S = rounded(S, dtype)
    Y = rounded(D * S, dtype)
    g = rounded(g, dtype)
    hp = high_precision(dtype)
    SY = sy_reference(S, Y, hp).value.astype(dtype).astype(F64)
    new = slots[-1]
    H = float(rounded(SY[new, new] / np.dot(Y[new], Y[new]), dtype))
    return {"S": S, "Y": Y, "SY": SY, "slots": slots, "g": g, "H": H}


def chronological(hist):
    """(S, Y, SY) of the selected pairs in chronological order."""
    sl = hist["slots"]
    return hist["S"][sl], hist["Y"][sl], hist["SY"][np.ix_(sl, sl)]


# The direction cases of tests/test_gpu_lbfgs_kernels.py; tests/test_lbfgs_oracle.py runs the same table through
# compact_direction.  Flags: g_offset = 1: g one element into its buffer; spike: also run with each of SPIKES;
# poison: also run with NaN in everything the call is specified not to use.
def _case(name, n, h, k, slots=None, **flags):
    return dict(name=name, n=n, h=h, k=k, slots=list(range(k)) if slots is None else slots, **flags)


DIRECTION_CASES = [
    _case("scalar-1", 1, 1, 1, spike=True),
    _case("scalar-3", 3, 2, 2, spike=True),
    _case("scalar-5", 5, 5, 3, spike=True),
    _case("scalar-255", 255, 8, 5, spike=True),
    _case("vector-odd-h", 256, 7, 7, spike=True),
    _case("vector-g-offset", 1024, 8, 6, g_offset=1, spike=True),
    _case("two-parts-scalar", 2049, 6, 6, spike=True),
    _case("two-parts-vector", 2052, 6, 6, spike=True),
    _case("parts-capped-by-rows", 12292, 128, 128, spike=True),
    _case("sixteen-parts", 30724, 5, 5, spike=True),
    _case("solve-63", 516, 128, 63),
    _case("solve-64", 516, 128, 64),
    _case("solve-65", 516, 128, 65),
    _case("solve-123", 516, 128, 123),
    _case("solve-124", 516, 128, 124),
    _case("solve-127", 516, 128, 127),
    _case("solve-128", 516, 128, 128),
    _case("ring-4-of-9", 300, 9, 4, slots=rotated_slots(9, 4, 7), poison=True),
    _case("ring-9-of-9", 300, 9, 9, slots=rotated_slots(9, 9, 3)),
    _case("ring-7-of-9", 300, 9, 7, slots=[8, 0, 2, 3, 5, 6, 7], poison=True),
    _case("ring-100-of-128", 516, 128, 100, slots=rotated_slots(128, 100, 60), poison=True),
]


@functools.lru_cache(maxsize=None)
def direction_case(name, dtype_name, spike=None):
    """(history, Val of the direction) of a table case; computed once per process and shared: treat as read-only."""
    case = next(c for c in DIRECTION_CASES if c["name"] == name)
    dtype = np.dtype(dtype_name).type
    hist = make_history(case["n"], case["h"], case["slots"], dtype, spike=spike)
    Sc, Yc, SYc = chronological(hist)
    val = direction_reference(Sc, Yc, hist["g"], hist["H"], dtype, SY=SYc.astype(dtype))
    for a in (hist["S"], hist["Y"], hist["SY"], hist["g"], val.value, val.mag):
        a.setflags(write=False)
    return hist, val
