"""Preconditioned CG on the GPU (recurrence 3, csrc/gpu/cg_pcg.hip): Jacobi and Chebyshev-polynomial
preconditioners on the generic CSR / SELL-64 engines, against the CPU oracle cpu_pcg (tests/test_precond.py
checks that one against numpy).

Reference anchors: the reference has no preconditioner (CUDACG.cu:269-352); the recurrence keeps its stop
test ||r||_2 < tol after the x / r update (:333), x0 = 0 and its iteration count (outer trips).
Shapes: the smallest that reach a tail tile (CSR: 256 rows), a tail slice (SELL: 64 rows) and several
blocks; bounds as tests/test_gpu_pipelined.py uses against its oracle.
"""
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

PRECONDS = [("jacobi", {}), ("chebyshev", {}), ("chebyshev", dict(cheb_degree=3, cheb_ratio=12.0))]


def scaled_laplacian(n=32, seed=7):
    """The n^2 5-point Laplacian scaled symmetrically by s_i = 10^(3 (u_i - 0.5)) (as tests/test_precond.py)."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    A = sp.kron(sp.identity(n), T) + sp.kron(T, sp.identity(n))
    s = 10.0 ** (3.0 * (np.random.default_rng(seed).random(n * n) - 0.5))
    A = (sp.diags(s) @ A @ sp.diags(s)).tocsr()
    A.sort_indices()
    return A, A @ np.ones(n * n)


def _spec(mcg, problem, kw):
    if problem == "scaled":
        A, b = scaled_laplacian()
        return mcg.csr_problem(A, b=b)
    return mcg.make_problem(problem, **kw)


_CPU = {}


def _cpu(mcg, problem, kw, precond, pkw, **okw):
    """cpu_pcg, computed once per (problem, preconditioner) and shared."""
    key = (problem, tuple(sorted(kw.items())), precond, tuple(sorted(pkw.items())), tuple(sorted(okw.items())))
    if key not in _CPU:
        C = mcg.native()
        o = C.CgOptions(maxit=2000, tol=1e-7)
        o.precond = precond
        for k, v in {**pkw, **okw}.items():
            setattr(o, k, v)
        _CPU[key] = C.cpu_cg(_spec(mcg, problem, kw).native(), o)
    return _CPU[key]


CASES = [
    ("poisson2d", dict(n=96), dict(format="csr"), "csr"),
    ("poisson2d", dict(n=50, coef=1), dict(format="sell16"), "sell64-d16"),  # 2500 rows: tail slice and tail tile
    ("poisson2d", dict(n=128, coef=1), dict(format="sellc8"), "sell64-d16"),  # no one-byte dictionary: d16
    ("poisson2d", dict(n=70), dict(format="sellc8"), "sell64-c8"),  # constant coefficients: the c8 codes
    ("poisson3d", dict(n=24, coef=1), dict(format="sell16"), "sell64-d16"),
    ("randspd", dict(rows=20000, band=40, density=0.4), dict(format="sell"), "sell64"),
    ("poisson2d", dict(n=50, coef=1), dict(format="csr", force_idx64=1), "csr"),
    ("randspd", dict(rows=20000, band=40, density=0.4), dict(format="csr"), "csr"),  # rows > 16: the adaptive engine
    ("scaled", {}, dict(format="sellc8"), None),
]


@pytest.mark.parametrize("precond,pkw", PRECONDS[:2])
@pytest.mark.parametrize("problem,kw,skw,fmt", CASES)
def test_pcg_matches_cpu_oracle(mcg, problem, kw, skw, fmt, precond, pkw):
    spec = _spec(mcg, problem, kw)
    s = mcg.CGSolver(spec, precond=precond, check_every=8, **pkw, **skw)
    i = s.info
    assert i["recurrence"] == "preconditioned" and i["precond"] == precond and i["fused_reduce"]
    assert not (i["carry"] or i["pmat"] or i["tiles"] or i["dia4"] or i["diav"] or i["ap_recompute"] or i["interleave"])
    assert fmt is None or i["format"] == fmt
    assert i["idx64"] == bool(skw.get("force_idx64"))
    if skw["format"] == "csr":  # thread per row while every row is short, else row-length adaptive tiles
        assert i["spmv_variant"] == (4 if problem == "randspd" else 1)
    m = 4 if precond == "chebyshev" else 1
    assert i["spmv_per_iteration"] == m and i["bytes_per_iter_model"] > 96 * i["n_local"]
    out = s.solve()
    cpu = _cpu(mcg, problem, kw, precond, pkw)
    print(f"{problem} {kw} {skw} {precond}: gpu {out['iterations']} cpu {cpu['iterations']} iterations")
    assert out["converged"] and cpu["converged"] and not out["breakdown"]
    assert abs(out["iterations"] - cpu["iterations"]) <= max(2, cpu["iterations"] // 100)
    np.testing.assert_allclose(out["x_local"], cpu["x"], rtol=1e-6, atol=1e-6 * np.abs(cpu["x"]).max())
    assert s.true_residual_norm() < 1e-6
    assert s.info["graph_fallbacks"] == 0 and s.info["graphs"]


def test_chebyshev_degrees_and_rtol(mcg):
    """degree 1 (no step), 2 (one step, z ends in the second buffer), 3 and 16; ratio / lmax; rtol."""
    problem, kw = "poisson2d", dict(n=50, coef=1)
    spec = _spec(mcg, problem, kw)
    for pkw in (dict(cheb_degree=1), dict(cheb_degree=2), dict(cheb_degree=3, cheb_ratio=12.0),
                dict(cheb_degree=16, cheb_lmax=2.2)):
        s = mcg.CGSolver(spec, precond="chebyshev", format="sell16", check_every=4, rtol=1e-9, **pkw)
        out = s.solve()
        cpu = _cpu(mcg, problem, kw, "chebyshev", pkw, rtol=1e-9)
        assert out["converged"] and cpu["converged"], pkw
        assert abs(out["iterations"] - cpu["iterations"]) <= max(2, cpu["iterations"] // 100), pkw
        np.testing.assert_allclose(out["x_local"], cpu["x"], rtol=1e-6, atol=1e-6 * np.abs(cpu["x"]).max())
        assert s.info["cheb_degree"] == pkw["cheb_degree"] and s.info["cheb_ratio"] == pkw.get("cheb_ratio", 30.0)
        if "cheb_lmax" in pkw:
            assert s.info["cheb_lmax"] == pkw["cheb_lmax"]


def _host(mcg, spec):
    A = mcg.models.to_scipy(spec)
    d = A.diagonal()
    return d, float((np.asarray(abs(A).sum(axis=1)).ravel() / d).max())


SCAN = [
    ("poisson2d", dict(n=50, coef=1), dict(format="csr")),
    ("poisson2d", dict(n=50, coef=1), dict(format="csr", force_idx64=1)),
    ("poisson2d", dict(n=50, coef=1), dict(format="sell")),
    ("poisson2d", dict(n=50, coef=1), dict(format="sell16")),
    ("poisson2d", dict(n=70), dict(format="sellc8")),
    ("randspd", dict(rows=3000, band=20, density=0.3), dict(format="sell16")),
    ("scaled", {}, dict(format="sellc8")),
]


@pytest.mark.parametrize("problem,kw,skw", SCAN)
def test_setup_scan_reads_the_stored_matrix(mcg, problem, kw, skw):
    spec = _spec(mcg, problem, kw)
    diag, gersh = _host(mcg, spec)
    s = mcg.CGSolver(spec, precond="chebyshev", **skw)
    np.testing.assert_array_equal(s.precond_dinv(), 1.0 / diag)
    assert abs(s.info["cheb_lmax"] - gersh) <= 1e-12 * gersh
    assert s.info["gershgorin"] == s.info["cheb_lmax"]
    if problem != "scaled":  # the project's diagonally dominant families
        assert 1.0 < gersh <= 2.0 + 1e-12


def test_setup_scan_through_sigma_sorted_slots(mcg):
    """SELL-C-sigma (a user matrix whose rows are sorted by length inside windows): the scan walks the
    stored slots and lands every row's reciprocal at its local row."""
    rng = np.random.default_rng(5)
    n = 1000
    B = sp.random(n, n, density=0.01, random_state=rng, format="csr")
    A = (B + B.T + sp.diags(np.asarray(abs(B + B.T).sum(axis=1)).ravel() + rng.random(n) + 0.5)).tocsr()
    A.sort_indices()
    spec = mcg.csr_problem(A, b=A @ np.ones(n))
    s = mcg.CGSolver(spec, precond="jacobi", format="sell", sell_sigma=128)
    assert s.info["sigma"] == 128
    np.testing.assert_array_equal(s.precond_dinv(), 1.0 / A.diagonal())
    out = s.solve()
    assert out["converged"] and np.linalg.norm(A @ out["x_local"] - A @ np.ones(n)) < 1e-6


@pytest.mark.parametrize("precond,pkw", PRECONDS)
@pytest.mark.parametrize("problem,kw,skw", [("poisson2d", dict(n=50, coef=1), dict(format="sell16")),
                                            ("poisson2d", dict(n=96), dict(format="csr"))])
def test_bitwise_repeatable_and_graph_equals_eager(mcg, problem, kw, skw, precond, pkw):
    spec = _spec(mcg, problem, kw)
    outs = [mcg.CGSolver(spec, precond=precond, use_graph=g, check_every=8, **pkw, **skw).solve()
            for g in (True, True, False)]
    for o in outs[1:]:
        assert o["iterations"] == outs[0]["iterations"] and o["rnorm"] == outs[0]["rnorm"]
        np.testing.assert_array_equal(o["x_local"], outs[0]["x_local"])


@pytest.mark.parametrize("precond,pkw", PRECONDS[:2])
def test_fixed_iterations_then_finalize_give_x_n(mcg, precond, pkw):
    """run_iterations(n) + finalize(): x_n and ||r_n|| of the oracle stopped at n.  The two differ by the
    order of their sums only: <= n eps = 2500 x 1.1e-16 = 3e-13 per dot product, 37 iterations of them
    (1e-11), amplified by at most the preconditioned condition number (~1e3 at 50^2): 1e-8."""
    problem, kw = "poisson2d", dict(n=50, coef=1)
    spec = _spec(mcg, problem, kw)
    cpu = _cpu(mcg, problem, kw, precond, pkw, maxit=37, tol=-1.0)
    s = mcg.CGSolver(spec, precond=precond, format="sell16", tol=-1.0, maxit=1 << 30, **pkw)
    s.reset()
    s.run(37)
    s.finalize()
    out = s.result()
    assert out["iterations"] == 37 and not out["converged"] and not out["breakdown"]
    assert abs(out["rnorm"] - cpu["rnorm"]) <= 1e-8 * cpu["rnorm"]
    np.testing.assert_allclose(s.x_local(), cpu["x"], rtol=1e-8, atol=1e-8 * np.abs(cpu["x"]).max())


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("precond,pkw", PRECONDS[:2])
def test_local_ranks_fixed_iterations_agree_with_one_rank(mcg, world, precond, pkw):
    spec = mcg.make_problem("poisson2d", n=128, coef=1)
    C = mcg.native()
    o = C.CgOptions(tol=-1.0, maxit=1 << 30, format="sell16")
    o.precond = precond
    key = ("one-rank", precond)
    if key not in _CPU:
        _CPU[key] = C.run_local_ranks(spec.native(), o, 1, 40, True)
    one = _CPU[key]
    many = C.run_local_ranks(spec.native(), o, world, 40, True)
    r1, rp = one["ranks"][0]["rnorm"], many["ranks"][0]["rnorm"]
    assert all(r["iterations"] == 40 for r in many["ranks"])
    assert abs(r1 - rp) <= 1e-9 * r1
    np.testing.assert_allclose(many["x"], one["x"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("precond,pkw", PRECONDS[:2])
@pytest.mark.parametrize("problem,kw,fmt", [("poisson2d", dict(n=64, coef=1), "sellc8"),
                                            ("poisson3d", dict(n=16, coef=1), "csr"),
                                            ("randspd", dict(rows=6000, band=30, density=0.3), "sell16")])
def test_local_ranks_match_cpu(mcg, world, problem, kw, fmt, precond, pkw):
    """P in-process ranks: halo of {z, p} before the pass and of z before every Chebyshev step, the two
    all-reduces, the Gershgorin bound agreed through the sum all-reduce, the latch agreement."""
    spec = mcg.make_problem(problem, **kw)
    C = mcg.native()
    cpu = _cpu(mcg, problem, kw, precond, pkw)
    o = C.CgOptions(maxit=2000, tol=1e-7, format=fmt, check_every=4)
    o.precond = precond
    out = C.run_local_ranks(spec.native(), o, world, 0, True)
    its = {r["iterations"] for r in out["ranks"]}
    assert len(its) == 1, its
    assert abs(its.pop() - cpu["iterations"]) <= max(2, cpu["iterations"] // 100)
    np.testing.assert_allclose(out["x"], cpu["x"], rtol=1e-6, atol=1e-6 * np.abs(cpu["x"]).max())
    assert all(r["true_rnorm"] < 1e-6 and r["converged"] for r in out["ranks"])


@pytest.mark.parametrize("precond", ["jacobi", "chebyshev"])
def test_inject_nan_latches_breakdown(mcg, precond):
    spec = mcg.make_problem("poisson2d", n=50, coef=1)
    s = mcg.CGSolver(spec, precond=precond, format="sell16", inject_nan_at=5, check_every=4)
    out = s.solve()
    assert out["breakdown"] and not out["converged"]
    assert out["iterations"] == 6  # the update of iteration 5 (0-based) reads the poisoned r; the next pass latches


def test_cli_prints_the_golden_lines(mcg):
    for extra in (["--precond", "jacobi"], ["--precond", "chebyshev", "--cheb-degree", "2"]):
        p = subprocess.run([mcg.cli_path()] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.stdout, p.stderr)
        assert p.stdout == "0.500000\n0.750000\n1.000000\nSuccess\n"


def test_solve_helper_and_default_unchanged(mcg):
    r = mcg.solve("poisson2d", n=64, coef=1, precond="jacobi")
    assert r["recurrence"] == "preconditioned" and r["precond"] == "jacobi" and r["converged"]
    plain = mcg.solve("poisson2d", n=64, coef=1, precond="none")
    assert plain["recurrence"] == "single-reduction" and plain["precond"] == "none" and plain["converged"]
    assert r["iterations"] <= 0.75 * plain["iterations"]
    i = mcg.CGSolver(mcg.make_problem("poisson2d", n=64, coef=1), precond="none").info
    assert i["carry"] and i["ap_recompute"] and i["diav"] and i["spmv_per_iteration"] == 1  # the lean-carry default


def test_refusals(mcg, tmp_path):
    C = mcg.native()
    spec = mcg.make_problem("poisson2d", n=64)
    for forced in (dict(carry=1), dict(pmat=1), dict(tiles=1), dict(interleave=1), dict(ap_recompute=1)):
        with pytest.raises(C.MCGError, match="cannot be forced"):
            mcg.CGSolver(spec, precond="jacobi", **forced)
    for rec in (0, 1, 2):
        with pytest.raises(ValueError, match="recurrence"):
            mcg.CGSolver(spec, precond="jacobi", recurrence=rec)
    o = C.CgOptions(format="sell16", recurrence=2)
    o.precond = 1
    with pytest.raises(C.MCGError, match="recurrence"):
        C.Solver(spec.native(), o)
    s = mcg.CGSolver(spec, precond="jacobi")
    with pytest.raises(C.MCGError, match="checkpoint"):
        s.save_checkpoint(str(tmp_path / "ck"))
    with pytest.raises(C.MCGError, match="checkpoint"):
        mcg.CGSolver(spec, precond="jacobi", checkpoint_every=8, checkpoint_path=str(tmp_path / "ck"))
    with pytest.raises(C.MCGError, match="no preconditioner"):
        mcg.CGSolver(spec).precond_dinv()
    # a bad diagonal: refused on one rank and, agreed through the all-reduce, on every rank of two
    A = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(400, 400)).tolil()
    A[300, 300] = -2.0
    bad = mcg.csr_problem(A.tocsr(), b=np.ones(400))
    with pytest.raises(C.MCGError, match="preconditioning needs a positive diagonal"):
        mcg.CGSolver(bad, precond="jacobi", format="csr")
    o = C.CgOptions(format="sell")
    o.precond = 2
    with pytest.raises(C.MCGError, match="preconditioning needs a positive diagonal"):
        C.run_local_ranks(bad.native(), o, 2, 0, False)
