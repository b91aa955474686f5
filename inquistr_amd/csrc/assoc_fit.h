// assoc_fit.h — the device steps the two `inquistr assoc` kernels share (assoc.hip: the ordinary fits; assoc_firth.hip: Firth's
// penalised logistic regression): the wave sums that leave the same bits in all 64 lanes, a sample's predictor, the moments the row
// filters and the centring need, and the Cholesky factorisation of a p x p matrix held as a lower triangle in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <type_traits>

#include "../../include/inquistr_hip.h"
#include "front_kernels.h"
#include "wave_primitives.h"

namespace inq {

constexpr double kAssocMuEps = 2.220446049250313e-16;  // 2^-52: mu stays in [eps, 1 - eps]
constexpr double kAssocRankTol = 1e-11;

// the sum over the 64 lanes, the same bits in every lane (all 64 lanes must be here)
__device__ __forceinline__ double wave_sum_f64(double x) {
    for (int d = 1; d < kWave; d *= 2) x += __shfl_xor(x, d, kWave);
    return x;
}
__device__ __forceinline__ double wave_min_f64(double x) {
    for (int d = 1; d < kWave; d *= 2) {
        const double o = __shfl_xor(x, d, kWave);
        x = o < x ? o : x;
    }
    return x;
}
__device__ __forceinline__ double wave_max_f64(double x) {
    for (int d = 1; d < kWave; d *= 2) {
        const double o = __shfl_xor(x, d, kWave);
        x = o > x ? o : x;
    }
    return x;
}

// pmax / pmin(H1, H2, na.rm = TRUE) and their mean: NaN only when both are
__device__ __forceinline__ double assoc_x(const float2 *row, uint32_t i, int mode) {
    const float2 h = row[i];
    const bool m1 = h.x != h.x, m2 = h.y != h.y;
    const float hi = m1 ? h.y : m2 ? h.x : (h.x > h.y ? h.x : h.y);
    const float lo = m1 ? h.y : m2 ? h.x : (h.x < h.y ? h.x : h.y);
    return mode == INQ_ASSOC_MAX ? (double)hi : mode == INQ_ASSOC_MIN ? (double)lo : ((double)hi + (double)lo) * 0.5;
}

// What the row filters and the centring need, from one pass over a row, the same in every lane
template <int P>
struct AssocMoments {
    uint32_t n, n1, n2;  // samples with an x; of them in group 1 / 2 (BINARY)
    double sx, s1, s2, mn, mx;
    double mean[P];  // [0] unused, [1] x, [2 + j] covariate j, over the samples with an x
};
template <int P, bool BINARY>
__device__ __forceinline__ AssocMoments<P> assoc_moments(const AssocArgs &a, const float2 *v, uint32_t lane) {
    constexpr int K = P - 2;
    const uint32_t ns = a.n_samples;
    const int mode = a.str_mode;
    uint32_t n = 0, n1 = 0, n2 = 0;
    double sx = 0.0, s1 = 0.0, s2 = 0.0, mn = INFINITY, mx = -INFINITY;
    AssocMoments<P> m;
#pragma unroll
    for (int j = 0; j < P; ++j) m.mean[j] = 0.0;  // sums first, then means
    for (uint32_t i = lane; i < ns; i += 64u) {
        const double x = assoc_x(v, i, mode);
        if (x != x) continue;
        ++n;
        sx += x;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        if (BINARY) {
            if (a.y[i] != 0.0) ++n2, s2 += x;
            else ++n1, s1 += x;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) m.mean[2 + j] += a.cov[(uint64_t)j * ns + i];
    }
    n = wave_sum_u32(n);
    sx = wave_sum_f64(sx);
    mn = wave_min_f64(mn);
    mx = wave_max_f64(mx);
    if (BINARY) {
        n1 = wave_sum_u32(n1), n2 = wave_sum_u32(n2);
        s1 = wave_sum_f64(s1), s2 = wave_sum_f64(s2);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) m.mean[2 + j] = wave_sum_f64(m.mean[2 + j]) / (double)n;
    m.mean[1] = sx / (double)n;
    m.n = n, m.n1 = n1, m.n2 = n2;
    m.sx = sx, m.s1 = s1, m.s2 = s2, m.mn = mn, m.mx = mx;
    return m;
}

__host__ __device__ constexpr int tix(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i, lower triangle by rows

// In place: M (lower triangle of a symmetric matrix) -> its Cholesky factor L.  False when a pivot is not above tol (NaN included);
// the factor is then unusable.
template <int P>
__device__ __forceinline__ bool cholesky(double (&M)[P * (P + 1) / 2], double tol) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        double d = M[tix(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= M[tix(j, k)] * M[tix(j, k)];
        ok = ok && d > tol;
        const double ljj = sqrt(d);
        M[tix(j, j)] = ljj;
#pragma unroll
        for (int i = j + 1; i < P; ++i) {
            double s = M[tix(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= M[tix(i, k)] * M[tix(j, k)];
            M[tix(i, j)] = s / ljj;
        }
    }
    return ok;
}
// L v = r
template <int P>
__device__ __forceinline__ void cholesky_forward(const double (&L)[P * (P + 1) / 2], const double (&r)[P], double (&v)[P]) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double s = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[tix(i, k)] * v[k];
        v[i] = s / L[tix(i, i)];
    }
}
// L' v = v, in place
template <int P>
__device__ __forceinline__ void cholesky_backward(const double (&L)[P * (P + 1) / 2], double (&v)[P]) {
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {
        double s = v[i];
#pragma unroll
        for (int k = i + 1; k < P; ++k) s -= L[tix(k, i)] * v[k];
        v[i] = s / L[tix(i, i)];
    }
}
// L L' v = r
template <int P>
__device__ __forceinline__ void cholesky_solve(const double (&L)[P * (P + 1) / 2], const double (&r)[P], double (&v)[P]) {
    cholesky_forward<P>(L, r, v);
    cholesky_backward<P>(L, v);
}

// go(std::integral_constant<int, p>) for p = 2 + k.  One kernel instantiation per p: p = 2 (no covariate, the common case) keeps 5
// accumulators, p = 8 keeps 44.  Rounding a smaller p up with zero columns would put zero pivots into the rank test
template <class F>
void assoc_for_p(uint32_t k, F &&go) {
    switch (k) {
    case 0: go(std::integral_constant<int, 2>{}); break;
    case 1: go(std::integral_constant<int, 3>{}); break;
    case 2: go(std::integral_constant<int, 4>{}); break;
    case 3: go(std::integral_constant<int, 5>{}); break;
    case 4: go(std::integral_constant<int, 6>{}); break;
    case 5: go(std::integral_constant<int, 7>{}); break;
    default: go(std::integral_constant<int, 8>{}); break;
    }
}

}  // namespace inq
