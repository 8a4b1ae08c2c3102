// Preconditioned CG (recurrence = 3): Jacobi and Chebyshev-polynomial preconditioners on D^-1 A.
//
// The reference has no preconditioner (CUDACG.cu:269-352 solves A x = b as it stands); this recurrence
// goes beyond it and keeps its conventions: x0 = 0, the absolute test ||r||_2 < tol on the recurrence
// residual after the x / r update (:333), no abort on non-positive curvature, iterations = outer trips.
//
//   x0 = 0, r0 = b, z0 = M r0, p0 = z0, rho0 = r0.z0
//   P_k  (SpMV, the engines of spmv_engines.hpp)  beta = rho_k / rho_{k-1};  p_k = z_k + beta p_{k-1}
//        recomputed in every gather (as k_cg_spmv_fused does with r);  q = A p_k;  partials of p_k.q
//   all-reduce
//   U_k  (elementwise, 16 B per lane)  alpha = rho_k / p.q;  x += alpha p_k;  r -= alpha q;  t = dinv o r
//        Jacobi: z = t, partials of {r.r, r.z};   Chebyshev: d = z = t / theta
//   C_j  (Chebyshev degree m: j = 1 .. m-1, SpMV gathering z)  d = c1_j d + c2_j dinv o (r - A z);  z += d
//        (z double-buffered in the ext layout; the last step takes {r.r, r.z}: r is read there anyway)
//   all-reduce
//
// so an outer iteration is 2 kernels (Jacobi) or m + 1 (Chebyshev) and 2 all-reduces whatever m.  Every
// kernel sums its block partials itself in a fixed order (f1_common.hpp last_arriver_reduce): no reduce
// launches, bitwise repeatable runs.  CgState: after P_k red[0] = p.q and rho = rho_k; after the
// iteration {red[0], red[1]} = {r.r, r.z}; the latch (converged / breakdown) is taken by P_{k+1}, which
// sees the all-reduced r.r of iteration k, or by cg_pcg_final after the last one.
//
// Bytes per row and outer iteration beside the matrix (ideal gathers): P reads z, p_{k-1} and writes p_k,
// q (32 B); U reads x, p, r, q, dinv and writes x, r, z (64 B; Chebyshev + d 8 B); C_j reads z, r, d, dinv
// and writes d, z (48 B) plus the matrix again.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "mcg/check.hpp"
#include "mcg/kernels.hpp"
#include "spmv_engines.hpp"

namespace mcg {
namespace kern {
namespace {

#include "f1_common.hpp"

struct PcgScalars {
  double beta;
  bool conv, bad;
};

// P_k's scalars from the all-reduced {r.r, r.z} of iteration k-1 and rho_{k-1}
__device__ __forceinline__ PcgScalars pcg_scalars(const CgState* st, double tol, int first, int check) {
  PcgScalars s;
  const double rr = st->red[0], rz = st->red[1];
  s.conv = check && sqrt(rr) < tol;  // the reference's break (CUDACG.cu:333)
  s.bad = check && !isfinite(rr);
  s.beta = first ? 0.0 : rz / st->rho;
  return s;
}

__device__ __forceinline__ void pcg_zero(CgState* st) {
  for (int q = 0; q < 4; ++q) st->red[q] = 0.0;
}

// last arriver of P_k: the latch on ||r_k||, or rotate rho and leave the local p.q for the all-reduce
__device__ __forceinline__ void pcg_book_pass(CgState* st, const BookSnap& s, const double* tot, int check, double tol) {
  if (s.done) {
    pcg_zero(st);
    return;
  }
  const double rr = s.red[0];
  const bool conv = check && sqrt(rr) < tol, bad = check && !isfinite(rr);
  if (conv || bad) {
    st->done = conv ? 1 : 3;
    st->converged = conv ? 1 : 0;
    st->breakdown = bad ? 1 : 0;
    st->conv_iter = s.iter;
    st->rr_final = rr;
    pcg_zero(st);
    return;
  }
  st->rho = s.red[1];
  st->rr_new = rr;
  st->red[0] = tot[0];
  st->red[1] = 0.0;
  st->red[2] = 0.0;
  st->red[3] = 0.0;
}

// last arriver of the iteration's last kernel: the local {r.r, r.z} for the all-reduce, one more iteration
__device__ __forceinline__ void pcg_book_iter(CgState* st, const BookSnap& s, const double* tot, int init) {
  if (s.done) {
    pcg_zero(st);
    return;
  }
  if (!init) {
    st->pAp = s.red[0];
    st->iter = s.iter + 1;
  }
  st->red[0] = tot[0];
  st->red[1] = tot[1];
  st->red[2] = 0.0;
  st->red[3] = 0.0;
}

__device__ __noinline__ void pcg_tail_pass(double* out, int pstride, RedCtl rc, CgState* st, double tol) {
  last_arriver_reduce<1>(
      out, pstride, rc, [&] { return book_snap(st); },
      [&](const double* t, const BookSnap& s) { pcg_book_pass(st, s, t, rc.check, tol); });
}

__device__ __noinline__ void pcg_tail_iter(double* out, int pstride, RedCtl rc, CgState* st) {
  last_arriver_reduce<2>(
      out, pstride, rc, [&] { return book_snap(st); },
      [&](const double* t, const BookSnap& s) { pcg_book_iter(st, s, t, rc.first); });
}

template <int FMT, typename IdxT, int U, class Gather, class Epi>
__device__ __forceinline__ void pcg_engine(const CsrDev<IdxT>& A, const SellDev& S, const TileRanges& tr, Gather&& gather,
                                           Epi&& epi) {
  if constexpr (FMT == 0) eng::csr_adaptive<IdxT, U, 16>(A, tr, gather, epi);
  else if constexpr (FMT == 6) eng::csr_direct<IdxT, U, false>(A, tr, gather, epi);
  else if constexpr (FMT == 1) eng::sell<U, false, 0>(S, tr, gather, epi);
  else if constexpr (FMT == 3) eng::sell<U, false, 1>(S, tr, gather, epi);
  else eng::sell<U, false, 2>(S, tr, gather, epi);
}

// P_k.  FMT: 0 CSR (row-length adaptive), 6 CSR (thread per row: every row short), 1 SELL-64, 3 SELL-64/d16,
// 4 SELL-64/c8
template <int FMT, typename IdxT, int U>
__global__ __launch_bounds__(kBS) void k_pcg_pass(CsrDev<IdxT> A, SellDev S, const double* __restrict__ z,
                                                  const double* __restrict__ pold, double* __restrict__ pnew,
                                                  double* __restrict__ q, int64_t own, TileRanges tr,
                                                  double* __restrict__ partials, int pstride, CgState* st, double tol,
                                                  RedCtl rc) {
  const PcgScalars sc = pcg_scalars(st, tol, rc.first, rc.check);
  double s_pq = 0.0;
  if (!st->done && !sc.conv && !sc.bad) {
    const double beta = sc.beta;
    auto gather = [&](int32_t c) { return fma(beta, pold[c], z[c]); };
    auto epi = [&](int64_t i, double sum) {
      const double pk = fma(beta, pold[own + i], z[own + i]);
      pnew[own + i] = pk;  // gathered by the next pass: a cached store
      st_stream(&q[i], sum);
      s_pq = fma(pk, sum, s_pq);
    };
    pcg_engine<FMT, IdxT, U>(A, S, tr, gather, epi);
  }
  block_partial4(s_pq, 0.0, 0.0, 0.0, partials, pstride, true);
  pcg_tail_pass(partials, pstride, rc, st, tol);
}

// C_j
template <int FMT, typename IdxT, int U, bool LAST>
__global__ __launch_bounds__(kBS) void k_pcg_cheb(CsrDev<IdxT> A, SellDev S, const double* __restrict__ zin,
                                                  double* __restrict__ zout, const double* __restrict__ r,
                                                  double* __restrict__ d, const double* __restrict__ dinv, double c1,
                                                  double c2, int64_t own, TileRanges tr, double* __restrict__ partials,
                                                  int pstride, CgState* st, RedCtl rc) {
  double s_rr = 0.0, s_rz = 0.0;
  if (!st->done) {
    auto gather = [&](int32_t c) { return zin[c]; };
    auto epi = [&](int64_t i, double sum) {
      const double ri = r[i];
      const double dn = fma(c1, d[i], c2 * (dinv[i] * (ri - sum)));
      const double zn = zin[own + i] + dn;
      d[i] = dn;
      zout[own + i] = zn;
      if constexpr (LAST) {
        s_rr = fma(ri, ri, s_rr);
        s_rz = fma(ri, zn, s_rz);
      }
    };
    pcg_engine<FMT, IdxT, U>(A, S, tr, gather, epi);
  }
  if constexpr (LAST) {
    block_partial4(s_rr, s_rz, 0.0, 0.0, partials, pstride, true);
    pcg_tail_iter(partials, pstride, rc, st);
  }
}

// U_k.  MODE 0 Jacobi, 1 Chebyshev degree 1, 2 Chebyshev (d = z, no sums).  V2: 16-B accesses (every vector
// 16-B aligned); INIT: alpha = 0 (x, p, q not touched: r = b on entry)
template <int MODE, bool V2, bool INIT>
__global__ __launch_bounds__(kBS) void k_pcg_update(double* __restrict__ x, double* __restrict__ r,
                                                    const double* __restrict__ q, const double* __restrict__ p,
                                                    const double* __restrict__ dinv, double* __restrict__ z,
                                                    double* __restrict__ d, int64_t n, double inv_theta,
                                                    double* __restrict__ partials, int pstride, CgState* st, RedCtl rc) {
  double s_rr = 0.0, s_rz = 0.0;
  if (!st->done) {
    const double alpha = INIT ? 0.0 : st->rho / st->red[0];
    const double na = -alpha;
    auto one = [&](double& xi, double& ri, double pi, double qi, double di, double& zi) {
      if constexpr (!INIT) {
        xi = fma(alpha, pi, xi);
        ri = fma(na, qi, ri);
      }
      const double t = di * ri;
      zi = MODE == 0 ? t : t * inv_theta;
      if constexpr (MODE != 2) {
        s_rr = fma(ri, ri, s_rr);
        s_rz = fma(ri, zi, s_rz);
      }
    };
    const int64_t stride = (int64_t)gridDim.x * kBS;
    const int64_t t0 = (int64_t)blockIdx.x * kBS + threadIdx.x;
    if constexpr (V2) {
      const int64_t n2 = n >> 1;
      double2* __restrict__ x2 = reinterpret_cast<double2*>(x);
      double2* __restrict__ r2 = reinterpret_cast<double2*>(r);
      const double2* __restrict__ q2 = reinterpret_cast<const double2*>(q);
      const double2* __restrict__ p2 = reinterpret_cast<const double2*>(p);
      const double2* __restrict__ i2 = reinterpret_cast<const double2*>(dinv);
      double2* __restrict__ z2 = reinterpret_cast<double2*>(z);
      double2* __restrict__ d2 = reinterpret_cast<double2*>(d);
      for (int64_t k = t0; k < n2; k += stride) {
        double2 xv = {0.0, 0.0}, pv = {0.0, 0.0}, qv = {0.0, 0.0}, zv;
        double2 rv = r2[k];
        const double2 dv = i2[k];
        if constexpr (!INIT) {
          xv = x2[k];
          pv = p2[k];
          qv = q2[k];
        }
        one(xv.x, rv.x, pv.x, qv.x, dv.x, zv.x);
        one(xv.y, rv.y, pv.y, qv.y, dv.y, zv.y);
        if constexpr (!INIT) {
          st_stream(&x2[k], xv);
          r2[k] = rv;
        }
        z2[k] = zv;
        if constexpr (MODE == 2) d2[k] = zv;
      }
      if ((n & 1) && t0 == 0) {
        const int64_t i = n - 1;
        double xi = INIT ? 0.0 : x[i], ri = r[i], zi;
        one(xi, ri, INIT ? 0.0 : p[i], INIT ? 0.0 : q[i], dinv[i], zi);
        if constexpr (!INIT) {
          x[i] = xi;
          r[i] = ri;
        }
        z[i] = zi;
        if constexpr (MODE == 2) d[i] = zi;
      }
    } else {
      for (int64_t i = t0; i < n; i += stride) {
        double xi = INIT ? 0.0 : x[i], ri = r[i], zi;
        one(xi, ri, INIT ? 0.0 : p[i], INIT ? 0.0 : q[i], dinv[i], zi);
        if constexpr (!INIT) {
          x[i] = xi;
          r[i] = ri;
        }
        z[i] = zi;
        if constexpr (MODE == 2) d[i] = zi;
      }
    }
  }
  if constexpr (MODE != 2) {
    block_partial4(s_rr, s_rz, 0.0, 0.0, partials, pstride, true);
    pcg_tail_iter(partials, pstride, rc, st);
  }
}

__global__ void k_pcg_final(CgState* st, double tol) {
  if (st->done) return;
  const double rr = st->red[0];
  st->done = 2;
  st->converged = sqrt(rr) < tol ? 1 : 0;
  st->breakdown = isfinite(rr) ? 0 : 1;
  st->conv_iter = st->iter;
  st->rr_final = rr;
}

// ---- setup scan: a_ii and sum_j |a_ij| of every stored row (not performance-critical) ----
template <typename IdxT>
__global__ __launch_bounds__(kBS) void k_pcg_scan_csr(CsrDev<IdxT> A, int64_t own, double* __restrict__ diag,
                                                      double* __restrict__ absum) {
  for (int64_t i = (int64_t)blockIdx.x * kBS + threadIdx.x; i < A.n_rows; i += (int64_t)gridDim.x * kBS) {
    double dd = 0.0, aa = 0.0;
    for (int64_t k = (int64_t)A.rowptr[i]; k < (int64_t)A.rowptr[i + 1]; ++k) {
      const double v = A.vals[k];
      if ((int64_t)A.cols[k] == own + i) dd += v;
      aa += fabs(v);
    }
    diag[i] = dd;
    absum[i] = aa;
  }
}

// one thread per SELL slot; CM as eng::sell_slice (0 int32 columns, 1 d16 offsets, 2 c8 codes)
template <int CM>
__global__ __launch_bounds__(kBS) void k_pcg_scan_sell(SellDev S, double* __restrict__ diag, double* __restrict__ absum) {
  for (int64_t i = (int64_t)blockIdx.x * kBS + threadIdx.x; i < S.n_rows; i += (int64_t)gridDim.x * kBS) {
    const int64_t sl = i >> 6, lane = i & 63;
    const int64_t base = S.slice_ptr[sl];
    const int w = (int)((S.slice_ptr[sl + 1] - base) >> 6);
    const int64_t row = S.perm ? (int64_t)S.perm[i] : i;
    const int32_t slotcol = (int32_t)(S.own_off + i);  // d16 / c8 offsets are relative to the slot's own column
    const int32_t dcol = (int32_t)(S.own_off + row);
    double dd = 0.0, aa = 0.0;
    for (int j = 0; j < w; ++j) {
      const int64_t e = base + (int64_t)j * 64 + lane;
      int32_t c;
      double v;
      if constexpr (CM == 2) {
        const double2 t = S.dict[S.codes[e]];
        c = slotcol + (int32_t)__double_as_longlong(t.y);
        v = t.x;
      } else if constexpr (CM == 1) {
        c = slotcol + (int32_t)S.dcols[e];
        v = S.vals[e];
      } else {
        c = S.cols[e];
        v = S.vals[e];
      }
      if (c == dcol) dd += v;  // (padding entries sit on the diagonal with value 0)
      aa += fabs(v);
    }
    diag[row] = dd;
    absum[row] = aa;
  }
}

// dinv in place of diag; per block {rows with a bad diagonal, max absum / diag} -> part[2 * grid]
__global__ __launch_bounds__(kBS) void k_pcg_dinv(double* __restrict__ dg, const double* __restrict__ absum, int64_t n,
                                                  double* __restrict__ part) {
  __shared__ double sh[2][kWaves];
  double bad = 0.0, mx = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBS + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBS) {
    const double dd = dg[i];
    if (!(dd > 0.0) || !isfinite(dd)) bad += 1.0;
    else mx = fmax(mx, absum[i] / dd);
    dg[i] = 1.0 / dd;
  }
  bad = eng::wave_sum(bad);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_down(mx, off, 64));
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = bad;
    sh[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double b = 0.0, m = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      b += sh[0][w];
      m = fmax(m, sh[1][w]);
    }
    part[blockIdx.x] = b;
    part[gridDim.x + blockIdx.x] = m;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

template <typename IdxT>
void pcg_scan(int fmt, const CsrDev<IdxT>& A, const SellDev& S, int64_t own_off, double* diag, double* absum,
              hipStream_t stream) {
  if (fmt == 6) fmt = 0;
  const int64_t n = fmt == 0 ? A.n_rows : S.n_rows;
  if (n <= 0) return;
  const int grid = (int)std::min<int64_t>((n + kBS - 1) / kBS, 8192);
  if (fmt == 0) hipLaunchKernelGGL(k_pcg_scan_csr<IdxT>, dim3(grid), dim3(kBS), 0, stream, A, own_off, diag, absum);
  else if (fmt == 1) hipLaunchKernelGGL(k_pcg_scan_sell<0>, dim3(grid), dim3(kBS), 0, stream, S, diag, absum);
  else if (fmt == 3) hipLaunchKernelGGL(k_pcg_scan_sell<1>, dim3(grid), dim3(kBS), 0, stream, S, diag, absum);
  else if (fmt == 4) hipLaunchKernelGGL(k_pcg_scan_sell<2>, dim3(grid), dim3(kBS), 0, stream, S, diag, absum);
  else fail("preconditioner setup: unsupported storage");
  MCG_HIP(hipGetLastError(), "kernel launch failed(pcg_scan)");
}
template void pcg_scan<int32_t>(int, const CsrDev<int32_t>&, const SellDev&, int64_t, double*, double*, hipStream_t);
template void pcg_scan<int64_t>(int, const CsrDev<int64_t>&, const SellDev&, int64_t, double*, double*, hipStream_t);

void pcg_dinv(double* diag_to_dinv, const double* absum, int64_t n, double* part, int grid, hipStream_t stream) {
  MCG_CHECK(grid >= 1, "pcg_dinv: empty grid");
  hipLaunchKernelGGL(k_pcg_dinv, dim3(grid), dim3(kBS), 0, stream, diag_to_dinv, absum, n, part);
  MCG_HIP(hipGetLastError(), "kernel launch failed(pcg_dinv)");
}

#define MCG_PCG_FMT(K, ...)                                   \
  do {                                                        \
    if (fmt == 0) {                                           \
      if (param <= 4) K(0, 4, __VA_ARGS__);                   \
      else K(0, 8, __VA_ARGS__);                              \
    } else if (fmt == 6) {                                    \
      if (param <= 4) K(6, 4, __VA_ARGS__);                   \
      else if (param <= 6) K(6, 6, __VA_ARGS__);              \
      else K(6, 8, __VA_ARGS__);                              \
    } else if (fmt == 1 || fmt == 3 || fmt == 4) {            \
      if (param <= 4) {                                       \
        if (fmt == 1) K(1, 4, __VA_ARGS__);                   \
        else if (fmt == 3) K(3, 4, __VA_ARGS__);              \
        else K(4, 4, __VA_ARGS__);                            \
      } else if (param <= 6) {                                \
        if (fmt == 1) K(1, 6, __VA_ARGS__);                   \
        else if (fmt == 3) K(3, 6, __VA_ARGS__);              \
        else K(4, 6, __VA_ARGS__);                            \
      } else {                                                \
        if (fmt == 1) K(1, 8, __VA_ARGS__);                   \
        else if (fmt == 3) K(3, 8, __VA_ARGS__);              \
        else K(4, 8, __VA_ARGS__);                            \
      }                                                       \
    } else {                                                  \
      fail("preconditioned CG: unsupported storage");         \
    }                                                         \
  } while (0)

template <typename IdxT>
void cg_pcg_pass(int fmt, int param, const CsrDev<IdxT>& A, const SellDev& S, const PcgVectors& v, int zsel,
                 int64_t own_off, const TileRanges& tr, double* partials, int pstride, int grid, CgState* st, double tol,
                 hipStream_t stream, const RedCtl& rc) {
  MCG_CHECK(grid >= 1 && rc.ngroups > 0 && rc.base == 0 && rc.cnt && rc.lvl2, "preconditioned CG: in-kernel reduction not set up");
  MCG_CHECK(v.p_old != v.p_new, "preconditioned CG: p_k needs a buffer of its own");
#define MCG_K(F, U, dummy)                                                                                            \
  hipLaunchKernelGGL((k_pcg_pass<F, IdxT, U>), dim3(grid), dim3(kBS), 0, stream, A, S, (const double*)v.z[zsel], v.p_old, \
                     v.p_new, v.q, own_off, tr, partials, pstride, st, tol, rc)
  MCG_PCG_FMT(MCG_K, 0);
#undef MCG_K
  MCG_HIP(hipGetLastError(), "compute mv failed(Ap)");
}
template void cg_pcg_pass<int32_t>(int, int, const CsrDev<int32_t>&, const SellDev&, const PcgVectors&, int, int64_t,
                                   const TileRanges&, double*, int, int, CgState*, double, hipStream_t, const RedCtl&);
template void cg_pcg_pass<int64_t>(int, int, const CsrDev<int64_t>&, const SellDev&, const PcgVectors&, int, int64_t,
                                   const TileRanges&, double*, int, int, CgState*, double, hipStream_t, const RedCtl&);

template <typename IdxT>
void cg_pcg_cheb_step(int fmt, int param, const CsrDev<IdxT>& A, const SellDev& S, const PcgVectors& v, int zin,
                      double c1, double c2, int last, int init, int64_t own_off, const TileRanges& tr, double* partials,
                      int pstride, int grid, CgState* st, hipStream_t stream, const RedCtl& rc_in) {
  MCG_CHECK(grid >= 1 && v.d && (zin == 0 || zin == 1), "Chebyshev step: bad arguments");
  RedCtl rc = rc_in;
  rc.first = init;  // pcg_book_iter: the initial sums count no iteration
  MCG_CHECK(!last || (rc.ngroups > 0 && rc.base == 0 && rc.cnt && rc.lvl2), "preconditioned CG: in-kernel reduction not set up");
#define MCG_K(F, U, L)                                                                                                 \
  hipLaunchKernelGGL((k_pcg_cheb<F, IdxT, U, L>), dim3(grid), dim3(kBS), 0, stream, A, S, (const double*)v.z[zin],     \
                     v.z[zin ^ 1], (const double*)v.r, v.d, v.dinv, c1, c2, own_off, tr, partials, pstride, st, rc)
  if (last) MCG_PCG_FMT(MCG_K, true);
  else MCG_PCG_FMT(MCG_K, false);
#undef MCG_K
  MCG_HIP(hipGetLastError(), "compute mv failed(z)");
}
template void cg_pcg_cheb_step<int32_t>(int, int, const CsrDev<int32_t>&, const SellDev&, const PcgVectors&, int, double,
                                        double, int, int, int64_t, const TileRanges&, double*, int, int, CgState*,
                                        hipStream_t, const RedCtl&);
template void cg_pcg_cheb_step<int64_t>(int, int, const CsrDev<int64_t>&, const SellDev&, const PcgVectors&, int, double,
                                        double, int, int, int64_t, const TileRanges&, double*, int, int, CgState*,
                                        hipStream_t, const RedCtl&);
#undef MCG_PCG_FMT

void cg_pcg_update(int mode, const PcgVectors& v, int64_t own_off, int64_t n, double inv_theta, int init,
                   double* partials, int pstride, int grid, CgState* st, hipStream_t stream, const RedCtl& rc_in) {
  MCG_CHECK(grid >= 1 && mode >= 0 && mode <= 2 && (mode != 2 || v.d), "preconditioned CG update: bad arguments");
  RedCtl rc = rc_in;
  rc.first = init;
  MCG_CHECK(mode == 2 || (rc.ngroups > 0 && rc.base == 0 && rc.cnt && rc.lvl2), "preconditioned CG: in-kernel reduction not set up");
  const double* p = v.p_new + own_off;
  double* z = v.z[0] + own_off;
  const bool v2 = aligned16(v.x) && aligned16(v.r) && aligned16(v.q) && aligned16(p) && aligned16(v.dinv) &&
                  aligned16(z) && aligned16(v.d);
#define MCG_K(M, V, I)                                                                                                \
  hipLaunchKernelGGL((k_pcg_update<M, V, I>), dim3(grid), dim3(kBS), 0, stream, v.x, v.r, (const double*)v.q, p, v.dinv, \
                     z, v.d, n, inv_theta, partials, pstride, st, rc)
#define MCG_M(M)                 \
  do {                           \
    if (v2) {                    \
      if (init) MCG_K(M, true, true);   \
      else MCG_K(M, true, false);       \
    } else {                     \
      if (init) MCG_K(M, false, true);  \
      else MCG_K(M, false, false);      \
    }                            \
  } while (0)
  if (mode == 0) MCG_M(0);
  else if (mode == 1) MCG_M(1);
  else MCG_M(2);
#undef MCG_M
#undef MCG_K
  MCG_HIP(hipGetLastError(), "compute axpy failed(r)");
}

void cg_pcg_final(CgState* st, double tol, hipStream_t stream) {
  hipLaunchKernelGGL(k_pcg_final, dim3(1), dim3(1), 0, stream, st, tol);
  MCG_HIP(hipGetLastError(), "compute norm2 failed(rho)");
}

}  // namespace kern
}  // namespace mcg
