"""Pins tests/lbfgs_oracle.py (the high-precision definition the GPU tests of the L-BFGS kernels compare with) without a
GPU: its two-loop recursion against sqfa_amd._lbfgs._History on the CPU and against a step of torch.optim.LBFGS, a plain
float32 numpy evaluation of the kernel's compact form against the bound in two summation orders, every planted mistake at
least 10x OUTSIDE the bound on every shape of the GPU table where it can be reached, and the branch predicates of
lbfgs_kernels.hip that the table's shapes were chosen by."""
import os
import re

import numpy as np
import pytest
import torch

import lbfgs_oracle as lo

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTSIDE = 10.0   # a planted mistake must land this many times outside the bound (issue: a condition, not a measurement)

VARIANTS = [(c["name"], sp) for c in lo.DIRECTION_CASES for sp in ((None,) + lo.SPIKES if c.get("spike") else (None,))]
CASE = {c["name"]: c for c in lo.DIRECTION_CASES}


def _id(v):
    return f"{v[0]}-{v[1] or 'plain'}"


# ---- the reference is the recursion the optimizer runs ---------------------------------------------------------------


@pytest.mark.skipif(not lo.LONGDOUBLE_OK, reason=lo.LONGDOUBLE_REASON)
@pytest.mark.parametrize("n,h,pushes", [(40, 5, 8), (300, 9, 9), (7, 3, 2), (129, 16, 30)])
def test_two_loop_is_the_history_class_on_the_cpu(n, h, pushes, monkeypatch):
    """_History without the native library (torch, float64, CPU: the compact form, SY from its own matrix products) against
    the two-loop recursion in long double on the pairs that survive in the ring, at the float64 bound."""
    from sqfa_amd._lbfgs import _History
    monkeypatch.setattr(_History, "native", False)
    k = min(h, pushes)
    hist = lo.make_history(n, pushes, list(range(pushes - k, pushes)), np.float64)
    ring = _History(h, torch.zeros(n, dtype=torch.float64))
    assert ring._lib is None
    for i in range(pushes):
        ring.push(torch.from_numpy(hist["Y"][i].copy()), torch.from_numpy(hist["S"][i].copy()))
    d = ring.direction(torch.from_numpy(hist["g"].copy()), hist["H"]).numpy()
    Sc, Yc, _ = lo.chronological(hist)
    assert np.array_equal(ring.S[ring.slots].numpy(), Sc) and np.array_equal(ring.Y[ring.slots].numpy(), Yc)
    SYc = ring.SY[ring.slots][:, ring.slots].numpy()
    sy = lo.sy_reference(Sc, Yc, lo.LD)
    assert lo.ratio(SYc, sy, np.float64) <= lo.C_FACTOR
    val = lo.direction_reference(Sc, Yc, hist["g"], hist["H"], np.float64, SY=SYc, sy_from="dots")
    assert lo.ratio(d, val, np.float64) <= lo.C_FACTOR


@pytest.mark.skipif(not lo.LONGDOUBLE_OK, reason=lo.LONGDOUBLE_REASON)
def test_two_loop_is_a_step_of_torch_lbfgs():
    """torch.optim.LBFGS with max_iter = 1 leaves the direction it took and everything it took it from in its state:
    the oracle's two-loop on those pairs reproduces `d` at the float64 bound (rho from the vectors: sy_from = "dots")."""
    torch.manual_seed(3)
    n = 24
    A = torch.randn(n, n, dtype=torch.float64)
    A = A @ A.T / n + torch.eye(n, dtype=torch.float64)
    x = torch.randn(n, dtype=torch.float64).requires_grad_()
    opt = torch.optim.LBFGS([x], lr=0.3, max_iter=1, history_size=5)

    def closure():
        opt.zero_grad()
        loss = 0.5 * x @ A @ x + 0.1 * (x ** 4).sum() + torch.cos(x).sum()
        loss.backward()
        return loss

    checked = 0
    for it in range(9):
        opt.step(closure)
        st = opt.state[opt._params[0]]
        if not st.get("old_stps"):
            continue
        S = np.stack([v.numpy() for v in st["old_stps"]])
        Y = np.stack([v.numpy() for v in st["old_dirs"]])
        g, H = st["prev_flat_grad"].numpy(), float(st["H_diag"])
        val = lo.direction_reference(S, Y, g, H, np.float64, sy_from="dots")
        assert lo.ratio(st["d"].numpy(), val, np.float64) <= lo.C_FACTOR, it
        checked += 1
    assert checked >= 7 and len(st["old_stps"]) == 5   # the history wrapped


def test_sy_reference_and_upper_inverse():
    rng = lo.rng_for(5)
    S, Y = rng.standard_normal((6, 37)), rng.standard_normal((4, 37))
    sy = lo.sy_reference(S, Y)
    assert sy.value.shape == (6, 4) and sy.n == 37 and np.allclose(sy.value, S @ Y.T, rtol=1e-14, atol=1e-14)
    assert np.allclose(sy.mag, np.abs(S) @ np.abs(Y).T) and (sy.mag >= np.abs(sy.value)).all()
    U = np.triu(rng.standard_normal((9, 9))) + 4 * np.eye(9)
    assert np.abs(lo.upper_inverse(U) @ U - np.eye(9)).max() < 1e-14
    assert np.abs(lo.upper_inverse(U.astype(lo.LD)).astype(np.float64) - np.linalg.inv(U)).max() < 1e-13


# ---- the histories are what their docstring says ---------------------------------------------------------------------


@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_histories_make_the_triangles_matter(variant):
    name, spike = variant
    hist, val = lo.direction_case(name, "float32", spike)
    Sc, Yc, SYc = lo.chronological(hist)
    k = len(hist["slots"])
    assert (np.diag(SYc) > 0).all() and hist["H"] > 0                      # curvature pairs
    # triu(SY) = (unit-scale banded triangle) diag(a): the column scales alone span SCALE_RANGE, a factor 8.8; measured <= 230
    assert np.linalg.cond(np.triu(SYc)) <= 1000
    assert np.isfinite(hist["S"]).all() and (hist["S"] != 0).all() and (hist["Y"] != 0).all()
    ratio_dg = np.linalg.norm(val.value) / np.linalg.norm(hist["g"])
    assert 0.1 <= ratio_dg <= 10.0
    if k >= 2:
        asym = np.abs(SYc - SYc.T).max() / np.abs(SYc).max()
        assert asym >= 0.05, asym                                          # measured: 0.1 ... 0.8
        # the history matters: without it the direction would be -H g (in a handful of dimensions the two can
        # coincide; with spikes the norms are those of the spikes)
        assert CASE[name]["n"] < 16 or spike or np.linalg.norm(val.value + hist["H"] * hist["g"]) >= 0.2 * np.linalg.norm(val.value)
    if spike:
        e = 0 if spike == "head" else CASE[name]["n"] - 1
        assert abs(hist["g"][e]) >= np.sqrt(CASE[name]["n"]) and abs(Sc[-1, e]) >= np.sqrt(CASE[name]["n"])


# ---- honest float32 arithmetic is inside the bound, mistakes are far outside -----------------------------------------


@pytest.mark.parametrize("order", ["sequential", "parts"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_float32_compact_form_stays_inside_the_bound(variant, order, record_property):
    name, spike = variant
    hist, val = lo.direction_case(name, "float32", spike)
    d = lo.compact_direction(hist["S"], hist["Y"], hist["SY"], hist["slots"], hist["g"], hist["H"], F32, order)
    r = lo.ratio(d, val, F32)
    record_property("ratio", r)
    assert r <= lo.C_FACTOR, r


MISTAKE_PARAMS = [(v, m) for v in VARIANTS for m in lo.MISTAKES
                  if lo.mistake_reachable(m, CASE[v[0]]["n"], CASE[v[0]]["slots"], v[1])]


@pytest.mark.parametrize("variant,mistake", MISTAKE_PARAMS, ids=lambda p: _id(p) if isinstance(p, tuple) else p)
def test_planted_mistake_lands_outside_the_bound(variant, mistake, record_property):
    name, spike = variant
    hist, val = lo.direction_case(name, "float32", spike)
    d = lo.compact_direction(hist["S"], hist["Y"], hist["SY"], hist["slots"], hist["g"], hist["H"], F32, "parts", mistake)
    r = lo.ratio(d, val, F32)
    record_property("ratio", r)
    assert r >= OUTSIDE * lo.C_FACTOR, r


def test_every_mistake_is_reached_somewhere_and_unreachable_ones_change_nothing():
    reached = {m for _, m in MISTAKE_PARAMS}
    assert reached == set(lo.MISTAKES)
    # every table shape with k >= 2 sees both triangle mistakes; every k % 4 != 0 both tails; every rotated ring the stale row
    for c in lo.DIRECTION_CASES:
        got = {m for (nm, sp), m in MISTAKE_PARAMS if nm == c["name"]}
        if c["k"] >= 2:
            assert {"transposed_triangle", "swapped_slots"} <= got
        if c["k"] % 4:
            assert "solve_tail_skipped" in got
        if c["slots"] != list(range(c["k"])):
            assert "stale_row" in got
        if c.get("spike") and c["n"] >= 2:
            assert {"dropped_first_element", "dropped_last_element"} <= got
    # where the tails are unreachable (k % 4 == 0) the option is a no-op of the evaluator
    hist, _ = lo.direction_case("solve-64", "float32")
    args = (hist["S"], hist["Y"], hist["SY"], hist["slots"], hist["g"], hist["H"], F32, "parts")
    clean = lo.compact_direction(*args)
    for m in ("solve_tail_skipped", "combine_tail_skipped"):
        assert np.array_equal(lo.compact_direction(*args, m), clean)


def test_step_stats_reference():
    rng = lo.rng_for(9)
    g, gp, d = (lo.rounded(rng.standard_normal(50), F32) for _ in range(3))
    y, s, val = lo.step_stats_reference(g, gp, d, 0.37, F32)
    assert y.dtype == F32 and np.array_equal(y, (g.astype(F32) - gp.astype(F32)))
    assert np.array_equal(s, F32(0.37) * d.astype(F32))
    y64, s64 = y.astype(np.float64), s.astype(np.float64)
    assert np.allclose(val.value, [np.abs(g).max(), np.abs(s64).max(), y64 @ s64, y64 @ y64, (y64 @ s64) / (y64 @ y64)], rtol=1e-14)
    got = np.array([val.value[0], val.value[1], F32(y @ s), F32(y @ y), F32(y @ s) / F32(y @ y)])
    assert lo.ratio(got, val, F32) <= lo.C_FACTOR


# ---- the branches the table's shapes were chosen by ------------------------------------------------------------------

LB_MAX_PARTS, LB_PART_MIN, LB_GRID_TARGET, LB_LDS_TRIANGLE_BYTES = 16, 2048, 768, 60 * 1024


def lb_parts(rows, n):
    """lbfgs_kernels.hip, lb_parts (the function under "parts a length-n dot product is split into")."""
    p = (LB_GRID_TARGET + rows - 1) // rows
    p = min(p, (n + LB_PART_MIN - 1) // LB_PART_MIN, LB_MAX_PARTS)
    return max(p, 1)


def lb_chunk(n, parts):
    """lbfgs_kernels.hip, launch_dots: chunk = ceil(n / parts) rounded up to a multiple of 4."""
    return ((n + parts - 1) // parts + 3) // 4 * 4


def in_lds(k, itemsize):
    """lbfgs_kernels.hip, launch_solve: tri_bytes <= 60 * 1024."""
    return k * (k + 1) // 2 * itemsize <= LB_LDS_TRIANGLE_BYTES


def r0_aligned(h):
    """lbfgs_kernels.hip, direction_impl: r0 = work + 2 h + 2 h LB_MAX_PARTS, and lb_vec_ok wants it 4 elements aligned
    (work itself is; so is every row of S and Y when n % 4 == 0)."""
    return (2 * h + 2 * h * LB_MAX_PARTS) % 4 == 0


def test_constants_restated_here_are_those_of_the_source():
    src = open(os.path.join(ROOT, "sqfa_amd", "csrc", "lbfgs_kernels.hip")).read()
    assert re.search(r"constexpr int LB_MAX_HISTORY = 128;", src)
    assert re.search(r"constexpr int LB_MAX_PARTS = 16;", src)
    assert re.search(r"constexpr int LB_PART_MIN = 2048;", src)
    assert re.search(r"int p = \(768 \+ rows - 1\) / rows;", src)
    assert re.search(r"const int in_lds = tri_bytes <= 60 \* 1024;", src)
    assert re.search(r"T\* r0 = work \+ 2 \* h \+ 2 \* \(size_t\)h \* LB_MAX_PARTS;", src)
    assert re.search(r"chunk = \(chunk \+ 3\) / 4 \* 4;", src)
    assert re.search(r"for \(int st = 0; st < k; st \+= 4\)", src) and re.search(r"for \(; i \+ 4 <= k; i \+= 4\)", src)
    from sqfa_amd import _lib
    lib = _lib.load()
    assert lib.sqfa_lbfgs_max_history() == lo.MAX_HISTORY
    for h, n in ((1, 1), (7, 256), (128, 12292), (5, 30724), (128, 516)):
        assert lib.sqfa_lbfgs_work_elems(h, n) == max(2 * h + 2 * h * LB_MAX_PARTS + n, 1024)


def test_table_shapes_reach_the_branches_they_are_listed_for():
    c = CASE
    parts = {name: lb_parts(v["k"], v["n"]) for name, v in c.items()}
    # one part, scalar dot products (n % 4 != 0)
    for name in ("scalar-1", "scalar-3", "scalar-5", "scalar-255"):
        assert parts[name] == 1 and c[name]["n"] % 4 != 0
    assert [c[n_]["k"] for n_ in ("scalar-1", "scalar-3", "scalar-5")] == [1, 2, 3]       # the group-of-four tails 1, 2, 3
    # vector dot products; odd h: r0 misaligned, the second product scalar
    assert c["vector-odd-h"]["n"] % 4 == 0 and not r0_aligned(c["vector-odd-h"]["h"]) and parts["vector-odd-h"] == 1
    assert c["vector-g-offset"]["n"] % 4 == 0 and r0_aligned(c["vector-g-offset"]["h"]) and c["vector-g-offset"]["g_offset"] == 1
    # two parts, the last chunk clipped
    for name, vec in (("two-parts-scalar", False), ("two-parts-vector", True)):
        n = c[name]["n"]
        chunk = lb_chunk(n, parts[name])
        assert parts[name] == 2 and chunk < n < 2 * chunk and (n % 4 == 0) == vec and r0_aligned(c[name]["h"])
    # parts capped by the rows (768 / rows), not by n or by 16; both products vector
    v = c["parts-capped-by-rows"]
    assert parts[v["name"]] == 6 == (768 + 127) // 128 < (v["n"] + 2047) // 2048 and v["n"] % 4 == 0 and r0_aligned(v["h"])
    assert lb_chunk(v["n"], 6) * 6 > v["n"]
    v = c["sixteen-parts"]
    assert parts[v["name"]] == 16 == (v["n"] + 2047) // 2048 and v["n"] % 4 == 0
    # the solve: second register row from k = 65, readlane boundary 63 / 64 / 65, the cap 128
    assert [c[f"solve-{k}"]["k"] for k in (63, 64, 65, 123, 124, 127, 128)] == [63, 64, 65, 123, 124, 127, 128]
    assert all(c[f"solve-{k}"]["h"] == 128 and parts[f"solve-{k}"] == 1 for k in (63, 64, 65, 123, 124, 127, 128))
    # float64 triangle: 123 in LDS, 124 not; float32 always
    assert in_lds(123, 8) and not in_lds(124, 8) and not in_lds(128, 8) and in_lds(128, 4)
    # wrapped rings
    for name in ("ring-4-of-9", "ring-9-of-9", "ring-7-of-9", "ring-100-of-128"):
        sl = c[name]["slots"]
        assert sl != sorted(sl) and len(set(sl)) == len(sl) == c[name]["k"] and max(sl) < c[name]["h"]
    assert sorted(c["ring-9-of-9"]["slots"]) == list(range(9)) and c["ring-4-of-9"]["k"] < 9
