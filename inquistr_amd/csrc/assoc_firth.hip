// assoc_firth.hip — Firth's penalised logistic regression for `inquistr assoc` (the model restated in
// include/inquistr_hip.h at inq_assoc_rows_firth): the fit for the loci whose maximum-likelihood estimate does not exist because
// the long alleles occur in one group only.  Runs behind assoc.hip's kernel on the same stream and reads what that left: a row's
// status and, for the fallback rule, the smallest min(mu, 1 - mu) of its last pass.  The choice of rows is made here: ONE WAVE PER
// LOCUS over all rows as in assoc.hip, and a wave whose row is not selected writes NOT_FITTED and returns.
// A selected row is fitted twice, all p coefficients free and with beta_x held at 0; each evaluation is two passes over the samples:
// A sums I = X'WX, every lane factors it; B takes each sample's hat value by a forward substitution with that factor and sums the
// modified score and the log-likelihood.  x is the LAST column here, so the leading (p - 1) x (p - 1) block of the one factor L is
// the factor of the null fit's free block and (I^-1)_xx = 1 / L[p-1][p-1]^2.  All sums end the same in all 64 lanes (assoc_fit.h), so
// every branch is wave-uniform: no LDS, no atomics, no barrier; every loop is bounded by a count known at entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <type_traits>

#include "../../include/inquistr_hip.h"
#include "assoc_fit.h"
#include "front_kernels.h"
#include "wave_primitives.h"

namespace inq {

namespace {

constexpr int kFirthMaxIter = 100;
constexpr double kFirthConverged = 1e-9;  // max_j |delta_j| sqrt(I_jj): a step in standard errors
constexpr double kFirthMaxStep = 5.0;

template <int P>
__global__ __launch_bounds__(256) void assoc_firth_kernel(AssocArgs a) {
    constexpr int K = P - 2, T = P * (P + 1) / 2, X = P - 1;  // X: x's column
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;  // the whole wave
    const double nan = __builtin_nan("");

    inq_assoc_firth_row_t out;
    out.beta = out.se = out.chi2 = out.p = out.pll_full = out.pll_null = nan;
    out.n_iter_full = out.n_iter_null = 0;
    out.status = INQ_ASSOC_FIRTH_ROW_NOT_FITTED;
#pragma unroll
    for (int j = 0; j < 5; ++j) out.pad[j] = 0;

    // every lane reads the same two words, so the choice is the wave's
    const uint8_t ordinary = a.rows[row].status;
    bool chosen = ordinary == INQ_ASSOC_ROW_OK || ordinary == INQ_ASSOC_ROW_NOT_CONVERGED;
    if (chosen && a.firth_when == INQ_ASSOC_FIRTH_FALLBACK)
        chosen = ordinary == INQ_ASSOC_ROW_NOT_CONVERGED || a.min_mu[row] < a.firth_mu_bound;
    if (!chosen) {
        if (lane == 0) a.firth[row] = out;
        return;
    }

    const uint32_t ns = a.n_samples;
    const float2 *v = reinterpret_cast<const float2 *>(a.values) + row * (uint64_t)ns;
    const int mode = a.str_mode;
    const AssocMoments<P> mo = assoc_moments<P, true>(a, v, lane);
    // a kept sample's centred columns [1, cov..., x], pi clamped as the ordinary fit clamps mu, and w
    auto sample = [&](uint32_t i, double x, const double (&beta)[P], double (&xc)[P], double &pi, double &w) {
        xc[0] = 1.0;
#pragma unroll
        for (int j = 0; j < K; ++j) xc[1 + j] = a.cov[(uint64_t)j * ns + i] - mo.mean[2 + j];
        xc[X] = x - mo.mean[1];
        double eta = beta[0];
#pragma unroll
        for (int j = 1; j < P; ++j) eta += beta[j] * xc[j];
        pi = 1.0 / (1.0 + exp(-eta));
        pi = pi < kAssocMuEps ? kAssocMuEps : pi > 1.0 - kAssocMuEps ? 1.0 - kAssocMuEps : pi;
        w = pi * (1.0 - pi);
    };

    int status = INQ_ASSOC_FIRTH_ROW_OK;
    double beta[P], M[T], pll[2] = {nan, nan};
    int steps[2] = {0, 0};
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {  // 0: the full fit, 1: the null fit
        const bool null_fit = which == 1;
#pragma unroll
        for (int j = 0; j < P; ++j) beta[j] = 0.0;
#pragma unroll 1
        for (int t = 0; t <= kFirthMaxIter; ++t) {
            // pass A: I(beta), its factor in every lane
#pragma unroll
            for (int j = 0; j < T; ++j) M[j] = 0.0;
            for (uint32_t i = lane; i < ns; i += 64u) {
                const double x = assoc_x(v, i, mode);
                if (x != x) continue;
                double xc[P], pi, w;
                sample(i, x, beta, xc, pi, w);
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const double wx = w * xc[p];
#pragma unroll
                    for (int q = 0; q <= p; ++q) M[tix(p, q)] += wx * xc[q];
                }
            }
#pragma unroll
            for (int j = 0; j < T; ++j) M[j] = wave_sum_f64(M[j]);
            double diag[P], top = M[tix(0, 0)];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                diag[j] = M[tix(j, j)];
                top = diag[j] > top ? diag[j] : top;
            }
            if (!cholesky<P>(M, kAssocRankTol * top)) {
                status = INQ_ASSOC_FIRTH_ROW_SINGULAR;
                break;
            }
            double logdet = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) logdet += log(M[tix(j, j)]);
            // pass B: hat values, the modified score, the log-likelihood
            double U[P], ll = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) U[j] = 0.0;
            for (uint32_t i = lane; i < ns; i += 64u) {
                const double x = assoc_x(v, i, mode);
                if (x != x) continue;
                double xc[P], u[P], pi, w;
                sample(i, x, beta, xc, pi, w);
                cholesky_forward<P>(M, xc, u);
                double h = 0.0;
#pragma unroll
                for (int j = 0; j < P; ++j) h += u[j] * u[j];
                h *= w;
                const double y = a.y[i];
                const double sc = (y - pi) + h * (0.5 - pi);
#pragma unroll
                for (int j = 0; j < P; ++j) U[j] += sc * xc[j];
                ll += log(y != 0.0 ? pi : 1.0 - pi);
            }
#pragma unroll
            for (int j = 0; j < P; ++j) U[j] = wave_sum_f64(U[j]);
            ll = wave_sum_f64(ll);
            pll[which] = ll + logdet;  // 1/2 log det I = sum log L_jj
            steps[which] = t;
            if (!(fabs(pll[which]) < INFINITY)) {
                status = INQ_ASSOC_FIRTH_ROW_NOT_CONVERGED;
                break;
            }
            // delta over the free coefficients: the null fit's free block is L's leading block
            double delta[P];
            cholesky_forward<P>(M, U, delta);
            if (null_fit) delta[X] = 0.0;
            cholesky_backward<P>(M, delta);
            double crit = 0.0, big = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const double d = fabs(delta[j]), c = d * sqrt(diag[j]);
                big = d > big ? d : big;
                crit = c > crit ? c : crit;
            }
            if (crit < kFirthConverged) break;
            if (t == kFirthMaxIter) {
                status = INQ_ASSOC_FIRTH_ROW_NOT_CONVERGED;
                break;
            }
            const double scale = big > kFirthMaxStep ? kFirthMaxStep / big : 1.0;
#pragma unroll
            for (int j = 0; j < P; ++j) beta[j] += delta[j] * scale;
        }
        if (status == INQ_ASSOC_FIRTH_ROW_SINGULAR) break;
        if (!null_fit) {
            out.beta = beta[X];
            out.se = 1.0 / M[tix(X, X)];
        }
    }
    if (status != INQ_ASSOC_FIRTH_ROW_SINGULAR) {
        const double d = 2.0 * (pll[0] - pll[1]);
        out.chi2 = d > 0.0 ? d : 0.0;
        out.p = erfc(sqrt(out.chi2 * 0.5));
        out.pll_full = pll[0], out.pll_null = pll[1];
        out.n_iter_full = (uint8_t)steps[0], out.n_iter_null = (uint8_t)steps[1];
    } else {
        out.beta = out.se = nan;
    }
    out.status = (uint8_t)status;
    if (lane == 0) a.firth[row] = out;
}

}  // namespace

void launch_assoc_firth(const AssocArgs &a, hipStream_t s) {
    if (!a.n_rows) return;
    const dim3 grid((uint32_t)((a.n_rows + 3) / 4));
    assoc_for_p(a.k, [&](auto p_c) { hipLaunchKernelGGL((assoc_firth_kernel<decltype(p_c)::value>), grid, dim3(256), 0, s, a); });
}

}  // namespace inq
