"""Preconditioned CG on the CPU (csrc/host/cpu_cg.cpp cpu_pcg): the oracle of the GPU's recurrence 3.

The reference solves the unpreconditioned system (CUDACG.cu:269-352); Jacobi and Chebyshev-polynomial
preconditioning go beyond it and keep its conventions (x0 = 0, the absolute test ||r||_2 < tol after the
x / r update, :333).  `np_pcg` below is an independent numpy / scipy statement of the same recurrence.
"""
import numpy as np
import pytest
import scipy.sparse as sp


def np_pcg(A, b, precond, m=4, ratio=30.0, lmax=0.0, tol=1e-7, maxit=2000):
    dinv = 1.0 / A.diagonal()
    if precond == "chebyshev":
        lmax = lmax or float((np.asarray(abs(A).sum(axis=1)).ravel() * dinv).max())  # Gershgorin bound of D^-1 A
        lmin = lmax / ratio
        theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
        sigma = theta / delta

    def M(r):
        if precond == "jacobi":
            return dinv * r
        d = dinv * r / theta
        z, rho = d.copy(), 1.0 / sigma
        for _ in range(1, m):
            rho_j = 1.0 / (2.0 * sigma - rho)
            d = rho_j * rho * d + (2.0 * rho_j / delta) * (dinv * (r - A @ z))
            z, rho = z + d, rho_j
        return z

    x, r = np.zeros_like(b), b.copy()
    z = M(r)
    p, rho = z.copy(), r @ z
    for k in range(maxit):
        q = A @ p
        alpha = rho / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) < tol:
            return x, k + 1, True
        z = M(r)
        rho_new = r @ z
        p, rho = z + (rho_new / rho) * p, rho_new
    return x, maxit, False


def scaled_laplacian(n=32, seed=7):
    """The n^2 5-point Laplacian scaled symmetrically by s_i = 10^(3 (u_i - 0.5)), u uniform: a user matrix
    with six decades of row scaling."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    A = sp.kron(sp.identity(n), T) + sp.kron(T, sp.identity(n))
    s = 10.0 ** (3.0 * (np.random.default_rng(seed).random(n * n) - 0.5))
    S = sp.diags(s)
    A = (S @ A @ S).tocsr()
    A.sort_indices()
    return A, A @ np.ones(n * n)


def _cpu(mcg, spec, **kw):
    C = mcg.native()
    o = C.CgOptions(maxit=kw.pop("maxit", 2000), tol=kw.pop("tol", 1e-7))
    for k, v in kw.items():
        setattr(o, k, v)
    return C.cpu_cg(spec.native(), o)


PROBLEMS = [("poisson2d", dict(n=64, coef=1)), ("poisson3d", dict(n=16, coef=1)), ("randspd", dict(rows=6000))]


@pytest.mark.parametrize("precond", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("problem,kw", PROBLEMS)
def test_cpu_pcg_matches_numpy(mcg, problem, kw, precond):
    spec = mcg.make_problem(problem, **kw)
    A, b = mcg.models.to_scipy(spec), mcg.models.rhs(spec)
    x, its, conv = np_pcg(A, b, precond)
    out = _cpu(mcg, spec, precond=precond)
    print(f"{problem} {precond}: cpu_pcg {out['iterations']} iterations, numpy {its}")
    assert conv and out["converged"] and not out["breakdown"]
    assert abs(out["iterations"] - its) <= max(2, its // 100)
    np.testing.assert_allclose(out["x"], x, rtol=1e-6, atol=1e-6 * np.abs(x).max())
    assert len(out["rnorm_history"]) == out["iterations"] and out["rnorm"] == out["rnorm_history"][-1]
    # cpu_cg dispatches to cpu_pcg
    direct = mcg.native().cpu_pcg(spec.native(), _o(mcg, precond=precond))
    assert direct["iterations"] == out["iterations"]
    np.testing.assert_array_equal(direct["x"], out["x"])


def _o(mcg, **kw):
    o = mcg.native().CgOptions(maxit=2000, tol=1e-7)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_chebyshev_parameters_reach_the_oracle(mcg):
    """degree, ratio and an explicit lmax: the same numbers in numpy."""
    spec = mcg.make_problem("poisson2d", n=32, coef=1)
    A, b = mcg.models.to_scipy(spec), mcg.models.rhs(spec)
    for m, ratio, lmax in [(1, 30.0, 0.0), (2, 10.0, 0.0), (6, 50.0, 2.5), (16, 30.0, 0.0)]:
        x, its, conv = np_pcg(A, b, "chebyshev", m=m, ratio=ratio, lmax=lmax)
        out = _cpu(mcg, spec, precond="chebyshev", cheb_degree=m, cheb_ratio=ratio, cheb_lmax=lmax)
        assert conv and out["converged"]
        assert abs(out["iterations"] - its) <= max(2, its // 100), (m, ratio, lmax)
        np.testing.assert_allclose(out["x"], x, rtol=1e-6, atol=1e-6 * np.abs(x).max())


def test_badly_scaled_user_matrix(mcg):
    A, b = scaled_laplacian()
    spec = mcg.csr_problem(A, b=b)
    plain = _cpu(mcg, spec)
    assert plain["iterations"] == 2000 and not plain["converged"]
    counts = {}
    for precond in ("jacobi", "chebyshev"):
        out = _cpu(mcg, spec, precond=precond)
        counts[precond] = out["iterations"]
        assert out["converged"], (precond, out["iterations"], out["rnorm"])
        assert np.linalg.norm(b - A @ out["x"]) < 1e-6
    print("scaled 32^2 Laplacian: plain rnorm", plain["rnorm"], "after 2000;", counts)


def test_iteration_counts_variable_coefficients(mcg):
    spec = mcg.make_problem("poisson2d", n=64, coef=1)
    plain = _cpu(mcg, spec)["iterations"]
    jac = _cpu(mcg, spec, precond="jacobi")["iterations"]
    cheb = _cpu(mcg, spec, precond="chebyshev", cheb_degree=4)["iterations"]
    print(f"64^2 coef=1: plain {plain}, jacobi {jac}, chebyshev-4 {cheb} (outer)")
    assert jac <= 0.75 * plain
    assert cheb <= 0.5 * jac


def test_rtol_and_python_entry_points(mcg):
    spec = mcg.make_problem("poisson2d", n=32, coef=1)
    b = mcg.models.rhs(spec)
    out = _cpu(mcg, spec, precond="jacobi", rtol=1e-6)
    assert out["converged"] and out["rnorm"] < 1e-6 * np.linalg.norm(b)
    assert out["rnorm_history"][-2] >= 1e-6 * np.linalg.norm(b)
    via = mcg.solve("poisson2d", device="cpu", n=32, coef=1, precond="chebyshev", cheb_degree=3)
    ref = _cpu(mcg, spec, precond="chebyshev", cheb_degree=3)
    assert via["iterations"] == ref["iterations"] and via["converged"]
    none = mcg.solve("poisson2d", device="cpu", n=32, coef=1, precond="none")
    assert none["iterations"] == _cpu(mcg, spec)["iterations"]


def test_option_errors(mcg):
    C = mcg.native()
    spec = mcg.make_problem("poisson2d", n=16)
    # a zero or negative diagonal
    for dval in (0.0, -2.0):
        A = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(20, 20)).tolil()
        A[7, 7] = dval
        bad = mcg.csr_problem(A.tocsr(), b=np.ones(20))
        with pytest.raises(C.MCGError, match="preconditioning needs a positive diagonal"):
            _cpu(mcg, bad, precond="jacobi")
    # an explicit recurrence
    for rec in (1, 2):
        with pytest.raises(C.MCGError, match="recurrence"):
            _cpu(mcg, spec, precond="jacobi", recurrence=rec)
    for rec in (0, 1, 2):
        with pytest.raises(ValueError, match="recurrence"):
            mcg.solve("poisson2d", device="cpu", n=16, precond="jacobi", recurrence=rec)
    # the degree
    for m in (0, 17, -1):
        with pytest.raises(C.MCGError, match="cheb_degree"):
            _cpu(mcg, spec, precond="chebyshev", cheb_degree=m)
    with pytest.raises(C.MCGError, match="cheb_ratio"):
        _cpu(mcg, spec, precond="chebyshev", cheb_ratio=1.0)
    with pytest.raises(C.MCGError, match="precond"):
        _cpu(mcg, spec, precond="ilu")
    # virtual ranks and checkpoints
    o = _o(mcg, precond="jacobi")
    with pytest.raises(C.MCGError, match="one rank"):
        C.cpu_cg_partitioned(spec.native(), 2, o)
    o.checkpoint_every = 10
    with pytest.raises(C.MCGError, match="checkpoint"):
        C.cpu_cg(spec.native(), o)


def test_cli_flags(mcg):
    import json
    import subprocess

    argv = ["--device", "cpu", "--problem", "poisson2d", "--n", "16", "--coef", "1", "--report", "json"]
    runs = {}
    for name, extra in [("plain", []), ("jacobi", ["--precond", "jacobi"]),
                        ("cheb", ["--precond", "chebyshev", "--cheb-degree", "3", "--cheb-ratio", "20"])]:
        p = subprocess.run([mcg.cli_path()] + argv + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and p.stdout.endswith("Success\n"), (p.stdout, p.stderr)
        runs[name] = json.loads(p.stdout.splitlines()[-2])
    assert "precond" not in runs["plain"]
    assert runs["jacobi"]["precond"] == "jacobi" and runs["cheb"]["precond"] == "chebyshev"
    assert runs["cheb"]["iterations"] < runs["jacobi"]["iterations"] <= runs["plain"]["iterations"]
    for extra in (["--precond", "jacobi", "--recurrence", "two"], ["--precond", "jacobi", "--sim-ranks", "2"],
                  ["--precond", "ilu"], ["--precond", "jacobi", "--checkpoint-every", "5"]):
        p = subprocess.run([mcg.cli_path()] + argv + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stdout.startswith("invalid arguments"), (extra, p.stdout)
