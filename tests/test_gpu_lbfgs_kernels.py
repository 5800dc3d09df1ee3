"""sqfa_lbfgs_push, sqfa_lbfgs_direction and sqfa_lbfgs_step_stats (sqfa_amd/csrc/lbfgs_kernels.hip) called straight through
the C ABI, against the high-precision definition in tests/lbfgs_oracle.py (pinned without a GPU by
tests/test_lbfgs_oracle.py): the two-loop recursion of torch.optim.LBFGS in float64 for the float32 kernels and in long
double for the float64 kernels -- a different algorithm from the compact form the kernels evaluate.

Every output AND the scratch `work` (exactly sqfa_lbfgs_work_elems(h, n) elements) is carved out of a larger buffer filled
with a sentinel; afterwards the margins must hold the sentinel's bit pattern, the inputs their own bits, and a second call
must give the same bits.  The direction gets S, Y and SY written by the test (SY from the oracle, rounded once), so an
error of the push can neither hide nor fake an error of the direction.  The comparison is elementwise,
|out - ref| <= 2 n u mag (lbfgs_oracle.ratio() <= C_FACTOR), with the composed first-order bound derived in the oracle's
docstring; the largest error / bound of each test is recorded (record_property "max_ratio").  The histories
(lbfgs_oracle.make_history) have a non-symmetric SY with off-diagonal entries as large as the diagonal, so that a
transposed triangle, exchanged slots, a skipped step, a stale row or (spike variants) a dropped first or last element is
an error of order one -- tests/test_lbfgs_oracle.py plants each of these in a numpy evaluation and finds it at least 10x
outside the bound on every shape below where it can occur.

Branch of lbfgs_kernels.hip -> case of lbfgs_oracle.DIRECTION_CASES (n, h, k) that takes it:

  lb_parts / launch_dots (test_direction, test_push)
    parts = 1 (n <= 2048)                        scalar-1 (1,1,1), scalar-3 (3,2,2), scalar-5 (5,5,3), scalar-255 (255,8,5),
                                                 vector-odd-h, vector-g-offset, solve-*, ring-*
    parts = 2, last chunk clipped                two-parts-scalar (2049,6,6: chunk 1028), two-parts-vector (2052,6,6: chunk 1028)
    parts capped by 768 / rows (6 < 7)           parts-capped-by-rows (12292,128,128); push at h = 128, n = 12292
    parts capped by LB_MAX_PARTS = 16            sixteen-parts (30724,5,5)
    parts capped by n / 2048 with rows small     push at h = 1 and 7, n = 2049 / 2052 (2 parts), n = 5 (1 part)
  lb_dots<T, true>  (n % 4 == 0, all aligned)    vector-odd-h first product, two-parts-vector, parts-capped-by-rows,
                                                 sixteen-parts first product, solve-*, ring-100-of-128, ring-* (n = 300)
  lb_dots<T, false> by n % 4 != 0                scalar-*, two-parts-scalar; push at n = 5, 2049
  lb_dots<T, false> by r0 = work + 34 h, h odd   vector-odd-h (256,7,7), sixteen-parts (h = 5), ring-* (h = 9): second product
  lb_dots<T, false> by a misaligned operand      vector-g-offset (1024,8,6) with g one element in (first product; the second
                                                 stays vector); push with s and y one element in (swap_src / v misaligned)
  lb_dots identity / swap_row (push only)        every test_push case: slot 0, h - 1 and the middle
  launch_solve, in_lds (every float32 k; float64 k <= 123)     all float32 cases; float64 up to solve-123
  launch_solve, triangle from global memory (float64 k >= 124) solve-124, solve-127, solve-128, parts-capped-by-rows in f64
  lb_solve upper / lower                         every direction call runs both
  lb_solve register row x1, readlane from it     solve-65 ... solve-128, ring-100-of-128, parts-capped-by-rows;
    boundary lanes 63 | 64                       solve-63 (x1 empty), solve-64 (last lane of x0), solve-65 (first of x1)
  lb_solve group-of-four tail, clamped reads     k % 4 = 1: scalar-1, scalar-255 (5), solve-65, sixteen-parts (5), ring-9-of-9
                                                 k % 4 = 2: scalar-3, vector-g-offset (6), two-parts-* (6)
                                                 k % 4 = 3: scalar-5, vector-odd-h (7), solve-63, solve-123, solve-127, ring-7-of-9
                                                 k % 4 = 0: solve-64, solve-124, solve-128, ring-4-of-9, ring-100-of-128
  lb_solve gather with pj >= h, pi stride        h = 1 ... 9 (most threads idle) and h = 128 (none idle)
  lb_combine groups of four + tail               the same k % 4 classes; post = H_diag (first call) and NULL (second call)
  lb_combine post == NULL in the FIRST call      test_direction_without_h_diag (H_diag = NULL against a tensor holding 1.0)
  k < h, ring order not the identity             ring-4-of-9, ring-7-of-9 (a subset with gaps), ring-9-of-9 (a rotation),
                                                 ring-100-of-128; scalar-5, scalar-255, vector-g-offset, solve-63 ... 127 (k < h,
                                                 ring not wrapped yet)
  lb_store_rows: row and column of SY, the diagonal entry written by two threads, the element blocks    test_push
  lb_step_stats / _finish: 1 block (n = 1, 1023), 5 blocks (n = 4100), every operand one element in     test_step_stats
  (256 blocks with several trips of the grid-stride loop: tests/test_gpu_lbfgs.py, n = 300001)
  host-side argument checks                      tests/test_cabi.py
"""
import ctypes

import numpy as np
import pytest
import torch

import lbfgs_oracle as lo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 64           # elements on either side of a buffer (a multiple of 32 bytes in both dtypes)
SENTINEL = -777.25
DTYPES = ["f32", "f64"]
NP = {"f32": np.float32, "f64": np.float64}
TORCH = {"f32": torch.float32, "f64": torch.float64}
INT = {"f32": torch.int32, "f64": torch.int64}
NAME = {"f32": "float32", "f64": "float64"}
CASE = {c["name"]: c for c in lo.DIRECTION_CASES}
VARIANTS = [(c["name"], sp) for c in lo.DIRECTION_CASES for sp in ((None,) + lo.SPIKES if c.get("spike") else (None,))]


def _vid(v):
    return f"{v[0]}-{v[1] or 'plain'}"


def _lib():
    from sqfa_amd import _lib as L
    return L


def _code(dt):
    return _lib().SQFA_F32 if dt == "f32" else _lib().SQFA_F64


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_reference(dt):
    if dt == "f64" and not lo.LONGDOUBLE_OK:
        pytest.skip(lo.LONGDOUBLE_REASON)


def _bits(t):
    return t.contiguous().view(-1).view(INT["f32" if t.dtype == torch.float32 else "f64"])


def dev(a, dt, mis=0):
    """Device tensor of the dtype under test holding `a`; mis = 1: one element into a buffer one element too long."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + mis, dtype=TORCH[dt], device=DEV)
    view = buf[mis:].view(a.shape)
    view.copy_(torch.from_numpy(a.astype(NP[dt])))
    assert view.is_contiguous() and view.data_ptr() % (4 * buf.element_size()) == (0 if not mis else buf.element_size())
    return view


class Guarded:
    """A buffer of `shape` inside a larger one: payload NaN (or `fill`) between margins that hold SENTINEL."""

    def __init__(self, shape, dt, fill=None, mis=0):
        n = int(np.prod(shape))
        self.dt, self.n, self.fill = dt, n, fill
        self.buf = torch.full((2 * MARGIN + n + mis,), SENTINEL, dtype=TORCH[dt], device=DEV)
        self.lo = MARGIN + mis
        self.view = self.buf[self.lo:self.lo + n].view(shape)
        self.pattern = int(torch.tensor([SENTINEL], dtype=TORCH[dt]).view(INT[dt]).item())
        self.reset()
        assert self.view.data_ptr() % (4 * self.buf.element_size()) == (0 if not mis else self.buf.element_size())

    def reset(self):
        if self.fill is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(self.fill).astype(NP[self.dt])))

    def check_margins(self):
        torch.cuda.synchronize()
        bits = self.buf.view(INT[self.dt])
        assert bool((bits[:self.lo] == self.pattern).all()), "write in front of the buffer"
        assert bool((bits[self.lo + self.n:] == self.pattern).all()), "write past the end of the buffer"

    def take(self, finite=True):
        """The payload on the host (dtype under test), after checking the margins; payload reset afterwards."""
        self.check_margins()
        out = self.view.detach().cpu().clone()
        if finite:
            assert bool(torch.isfinite(out).all()), "an output element was not written (or is not finite)"
        self.reset()
        return out


def run_twice(launch, outs, scratch=()):
    """Launch, collect, launch again: margins intact, both results the same bits.  Returns numpy arrays of the dtype."""
    first = None
    for _ in range(2):
        launch()
        for s in scratch:
            s.check_margins()
            s.reset()
        got = [o.take() for o in outs]
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                assert torch.equal(_bits(a), _bits(b)), "two calls differ"
    return [g.numpy() for g in first]


def check(out, val, dt, worst):
    r = lo.ratio(out, val, NP[dt])
    worst.append(r)
    assert r <= lo.C_FACTOR, f"error / (n u magnitude) = {r:.3g} > {lo.C_FACTOR}"


# ---- direction -----------------------------------------------------------------------------------------------------


def run_direction(hist, dt, g_mis=0, H="given", poison=False):
    """d_out of sqfa_lbfgs_direction on the ring buffers of `hist`.  H: "given" (hist["H"] in a device scalar), None (NULL)
    or a float.  poison: NaN in every row of S / Y outside the slots and every SY entry outside their rows x columns."""
    L = _lib()
    lib = L.load()
    S, Y, SY = np.array(hist["S"]), np.array(hist["Y"]), np.array(hist["SY"])
    h, n = S.shape
    slots = list(hist["slots"])
    k = len(slots)
    if poison:
        unused = [r for r in range(h) if r not in slots]
        assert unused
        S[unused] = np.nan
        Y[unused] = np.nan
        keep = np.zeros((h, h), dtype=bool)
        keep[np.ix_(slots, slots)] = True
        SY[~keep] = np.nan
    Sd, Yd, SYd, gd = dev(S, dt), dev(Y, dt), dev(SY, dt), dev(hist["g"], dt, g_mis)
    Hd = None if H is None else dev(np.array([hist["H"] if H == "given" else H]), dt)
    before = [_bits(t).clone() for t in (Sd, Yd, SYd, gd)]
    work_elems = lib.sqfa_lbfgs_work_elems(h, n)
    assert work_elems == max(34 * h + n, 1024)
    d, work = Guarded((n,), dt), Guarded((work_elems,), dt)
    c_slots = (ctypes.c_int * k)(*slots)

    def launch():
        rc = lib.sqfa_lbfgs_direction(_ptr(Sd), _ptr(Yd), _ptr(SYd), h, n, c_slots, k, _ptr(gd), _ptr(Hd), _ptr(d.view),
                                      _ptr(work.view), _code(dt), _stream())
        assert rc == L.SQFA_OK, rc

    (out,) = run_twice(launch, [d], scratch=[work])
    for t, b in zip((Sd, Yd, SYd, gd), before):
        assert torch.equal(_bits(t), b), "an input was written"
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_direction(variant, dt, record_property):
    """Every case of the table (module docstring), plain and with head / tail spikes, against the two-loop recursion."""
    _need_reference(dt)
    name, spike = variant
    hist, val = lo.direction_case(name, NAME[dt], spike)
    worst = []
    check(run_direction(hist, dt), val, dt, worst)
    if CASE[name].get("g_offset"):
        # n % 4 == 0 but g not 16-byte aligned: the scalar kernel must be taken, with the same result to the bound
        check(run_direction(hist, dt, g_mis=1), val, dt, worst)
    record_property("max_ratio", max(worst))


@pytest.mark.parametrize("dt", DTYPES)
def test_direction_without_h_diag(dt, record_property):
    """H_diag = NULL is H = 1: the same bits as a device scalar holding 1.0, and the oracle's direction for H = 1."""
    _need_reference(dt)
    hist, _ = lo.direction_case("ring-9-of-9", NAME[dt])
    null, one = run_direction(hist, dt, H=None), run_direction(hist, dt, H=1.0)
    assert np.array_equal(null.view(np.int32 if dt == "f32" else np.int64), one.view(np.int32 if dt == "f32" else np.int64))
    Sc, Yc, SYc = lo.chronological(hist)
    val = lo.direction_reference(Sc, Yc, hist["g"], 1.0, NP[dt], SY=SYc.astype(NP[dt]))
    worst = []
    check(null, val, dt, worst)
    record_property("max_ratio", max(worst))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in lo.DIRECTION_CASES if c.get("poison")])
def test_direction_ignores_what_is_not_listed(name, dt):
    """The guarantee of include/sqfa_hip.h: rows of S / Y outside `slots` and SY entries outside their rows x columns may
    hold anything.  NaN there (memory the call is specified not to use), and d_out is the same bits as with finite values."""
    hist, _ = lo.direction_case(name, NAME[dt]) if (dt == "f32" or lo.LONGDOUBLE_OK) else (
        lo.make_history(CASE[name]["n"], CASE[name]["h"], CASE[name]["slots"], NP[dt]), None)
    clean, dirty = run_direction(hist, dt), run_direction(hist, dt, poison=True)
    as_int = np.int32 if dt == "f32" else np.int64
    assert np.array_equal(clean.view(as_int), dirty.view(as_int))


# ---- push ----------------------------------------------------------------------------------------------------------

PUSH_CASES = sorted({(h, n, slot) for h in (1, 7, 128) for n in (5, 2049, 2052) for slot in (0, h // 2, h - 1)} | {(128, 12292, 77)})


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("h,n,slot,mis", [c + (m,) for c in PUSH_CASES for m in ((0, 1) if c[1] < 4096 else (0,))])
def test_push(h, n, slot, mis, dt, record_property):
    """Rows `slot` of S / Y are s / y bit for bit and every other row keeps its bits; row and column `slot` of SY (the
    diagonal entry included) meet the dot-product bound against the oracle and every other entry keeps its bits.
    mis = 1: s and y one element into their buffers (the scalar kernel), the same result to the bound."""
    _need_reference(dt)
    L = _lib()
    lib = L.load()
    dtype = NP[dt]
    rng = lo.rng_for(31, h, n, slot)
    S0, Y0 = lo.rounded(rng.standard_normal((h, n)), dtype), lo.rounded(rng.standard_normal((h, n)), dtype)
    SY0 = lo.rounded(rng.standard_normal((h, h)), dtype)
    s = lo.rounded(rng.standard_normal(n), dtype)
    y = lo.rounded(s * (1.0 + 0.5 * rng.random(n)) + 0.3 * rng.standard_normal(n), dtype)
    S, Y, SY = Guarded((h, n), dt, fill=S0), Guarded((h, n), dt, fill=Y0), Guarded((h, h), dt, fill=SY0)
    work = Guarded((lib.sqfa_lbfgs_work_elems(h, n),), dt)
    sd, yd = dev(s, dt, mis), dev(y, dt, mis)

    def launch():
        rc = lib.sqfa_lbfgs_push(_ptr(S.view), _ptr(Y.view), _ptr(SY.view), h, n, slot, _ptr(sd), _ptr(yd), _ptr(work.view),
                                 _code(dt), _stream())
        assert rc == L.SQFA_OK, rc

    S1, Y1, SY1 = run_twice(launch, [S, Y, SY], scratch=[work])
    assert torch.equal(sd.cpu(), torch.from_numpy(s.astype(dtype))) and torch.equal(yd.cpu(), torch.from_numpy(y.astype(dtype)))
    S_ref, Y_ref = S0.copy(), Y0.copy()
    S_ref[slot], Y_ref[slot] = s, y
    assert np.array_equal(S1, S_ref.astype(dtype)) and np.array_equal(Y1, Y_ref.astype(dtype))
    other = np.ones((h, h), dtype=bool)
    other[slot, :] = False
    other[:, slot] = False
    assert np.array_equal(SY1[other], SY0.astype(dtype)[other]), "an SY entry outside row and column `slot` changed"
    hp = lo.high_precision(dtype)
    row = lo.sy_reference(s[None, :], Y_ref, hp)      # SY[slot][j] = s . y_j
    col = lo.sy_reference(S_ref, y[None, :], hp)      # SY[i][slot] = s_i . y
    worst = []
    check(SY1[slot, :][None, :], row, dt, worst)
    check(SY1[:, slot][:, None], col, dt, worst)
    record_property("max_ratio", max(worst))


@pytest.mark.parametrize("dt", DTYPES)
def test_history_chain(dt, record_property):
    """Ring bookkeeping and kernels together, once: h + 3 pairs pushed through sqfa_amd._lbfgs._History with h = 5, then the
    direction against the two-loop recursion on the five pairs that survive (SY from the push: sy_from = "dots")."""
    _need_reference(dt)
    from sqfa_amd._lbfgs import _History
    n, h, pushes = 300, 5, 8
    dtype = NP[dt]
    hist = lo.make_history(n, pushes, list(range(pushes - h, pushes)), dtype)
    ring = _History(h, torch.zeros(n, dtype=TORCH[dt], device=DEV))
    assert ring._lib is not None
    for i in range(pushes):
        ring.push(dev(hist["Y"][i], dt), dev(hist["S"][i], dt))
    assert ring.slots == [3, 4, 0, 1, 2]
    d = ring.direction(dev(hist["g"], dt), dev(np.array(hist["H"]), dt).reshape(()))
    torch.cuda.synchronize()
    Sc, Yc, _ = lo.chronological(hist)
    assert np.array_equal(ring.S[ring.slots].cpu().numpy(), Sc.astype(dtype))
    assert np.array_equal(ring.Y[ring.slots].cpu().numpy(), Yc.astype(dtype))
    SYc = ring.SY[ring.slots][:, ring.slots].cpu().numpy()
    worst = []
    check(SYc, lo.sy_reference(Sc, Yc, lo.high_precision(dtype)), dt, worst)
    val = lo.direction_reference(Sc, Yc, hist["g"], hist["H"], dtype, SY=SYc, sy_from="dots")
    check(d.cpu().numpy(), val, dt, worst)
    record_property("max_ratio", max(worst))


# ---- step stats ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("n", [1, 1023, 4100])
def test_step_stats(n, mis, dt, record_property):
    """y = g - g_prev and s = t d bit for bit, the five scalars to the bound (the maxima exactly), nothing written outside
    y_out, s_out, the five scalars and `work`; mis = 1: g, g_prev and d one element into their buffers."""
    _need_reference(dt)
    L = _lib()
    lib = L.load()
    dtype = NP[dt]
    rng = lo.rng_for(41, n)
    g, gp, d = (lo.rounded(rng.standard_normal(n), dtype) for _ in range(3))
    t = 0.37
    y_ref, s_ref, val = lo.step_stats_reference(g, gp, d, t, dtype)
    gd, gpd, dd = dev(g, dt, mis), dev(gp, dt, mis), dev(d, dt, mis)
    y, s, scal = Guarded((n,), dt), Guarded((n,), dt), Guarded((5,), dt)
    work = Guarded((lib.sqfa_lbfgs_work_elems(1, n),), dt)

    def launch():
        rc = lib.sqfa_lbfgs_step_stats(_ptr(gd), _ptr(gpd), _ptr(dd), t, n, _ptr(y.view), _ptr(s.view), _ptr(scal.view),
                                       _ptr(work.view), _code(dt), _stream())
        assert rc == L.SQFA_OK, rc

    y1, s1, scal1 = run_twice(launch, [y, s, scal], scratch=[work])
    assert np.array_equal(y1, y_ref) and np.array_equal(s1, s_ref)
    worst = []
    check(scal1, val, dt, worst)
    record_property("max_ratio", max(worst))
