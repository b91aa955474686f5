// assoc.hip — `inquistr assoc` on the GPU: one regression per locus of a combined .inq, the model of the
// reference's scripts/STR_regression.R (one glm() per locus in an R loop) restated in include/inquistr_hip.h.
// Loci are independent and small (a few hundred samples, p = 2 ... 8 columns): ONE WAVE PER LOCUS, four loci per workgroup.
// Lane l takes samples l, l + 64, ...: a sample's H1 / H2 are one 8-byte load, a wave reads 512 contiguous bytes of its row per
// step.  y and the covariates are shared by every wave (L2).  Each pass over the samples leaves the lower triangle of X'WX, X'Wz
// and the deviance in f64 registers of every lane; a butterfly of adds leaves the SAME sums in all 64 lanes (a + b == b + a, bit
// for bit), so every lane does the p x p Cholesky solve and every branch on its results is wave-uniform: no LDS, no atomics, no
// barrier.  Every non-intercept column is centred on its mean over the row's kept samples first: that changes neither beta_x nor
// its standard error and keeps lengths like 10 000 +- 1 well conditioned.  Every loop is bounded by a count known at entry.
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

constexpr int kAssocMaxIter = 25;                    // glm.control(maxit = 25)
constexpr double kAssocConverged = 1e-8;             // glm.control(epsilon = 1e-8)
constexpr int kBetaCfMaxIter = 1000;  // Lentz: about sqrt(max(a, b)) steps are needed, a = df / 2 <= 32 768

// Continued fraction of the incomplete beta function by the modified Lentz method
__device__ double beta_cf(double a, double b, double x) {
    const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= kBetaCfMaxIter; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-16) break;
    }
    return h;
}

// Two-sided Student-t p: I_x(df / 2, 1 / 2) at x = df / (df + t^2); coef = 1 / B(df / 2, 1 / 2) (AssocArgs::tcoef)
__device__ double student_t_two_sided(double t, double df, double coef) {
    if (t != t) return t;
    const double t2 = t * t;
    if (t2 == INFINITY) return 0.0;
    if (t2 == 0.0) return 1.0;
    const double a = 0.5 * df, b = 0.5;
    const double x = df / (df + t2), xc = t2 / (df + t2);  // xc = 1 - x without the cancellation
    const double front = coef * exp(-a * log1p(t2 / df)) * sqrt(xc);  // x^a (1 - x)^b / B(a, b)
    if (x < (a + 1.0) / (a + b + 2.0)) return front * beta_cf(a, b, x) / a;
    return 1.0 - front * beta_cf(b, a, xc) / b;
}

template <int P, bool BINARY>
__global__ __launch_bounds__(256) void assoc_kernel(AssocArgs a) {
    constexpr int K = P - 2, T = P * (P + 1) / 2;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;  // the whole wave: the lanes of a wave that stays all reach every butterfly below
    const uint32_t ns = a.n_samples;
    const float2 *v = reinterpret_cast<const float2 *>(a.values) + row * (uint64_t)ns;
    const int mode = a.str_mode;
    const double nan = __builtin_nan("");

    // pass 0: what the filters and the centring need
    const AssocMoments<P> mo = assoc_moments<P, BINARY>(a, v, lane);
    const uint32_t n = mo.n, n1 = mo.n1, n2 = mo.n2;
    const double sx = mo.sx, s1 = mo.s1, s2 = mo.s2, mn = mo.mn, mx = mo.mx;
    const double (&mean)[P] = mo.mean;

    inq_assoc_row_t out;
    out.beta = out.se = out.stat = out.p = nan;
    out.mean_all = n ? mean[1] : nan;
    out.mean_g1 = BINARY && n1 ? s1 / (double)n1 : nan;
    out.mean_g2 = BINARY && n2 ? s2 / (double)n2 : nan;
    out.min_x = n ? mn : nan;
    out.max_x = n ? mx : nan;
    out.n = n, out.n_g1 = n1, out.n_g2 = n2;
    out.status = INQ_ASSOC_ROW_OK, out.n_iter = 0;
    out.pad[0] = out.pad[1] = 0;

    if (!((double)n / (double)ns >= a.missing_cutoff)) out.status = INQ_ASSOC_ROW_LOW_CALL_RATE;
    else if (!(mn != mx)) out.status = INQ_ASSOC_ROW_CONSTANT;
    else if (BINARY && (!n1 || !n2)) out.status = INQ_ASSOC_ROW_ONE_GROUP;
    else if (n <= (uint32_t)P) out.status = INQ_ASSOC_ROW_TOO_FEW;
    else if (!(fabs(sx) < INFINITY)) out.status = INQ_ASSOC_ROW_SINGULAR;  // an infinite x: its centred column is not finite
    if (out.status != INQ_ASSOC_ROW_OK) {
        if (lane == 0) a.rows[row] = out;
        return;
    }

    double beta[P], inv_xx = nan;
#pragma unroll
    for (int j = 0; j < P; ++j) beta[j] = 0.0;
    // one pass over the kept samples: M += w xc xc', r += w xc z for what `each` makes of a sample (false: no contribution), then
    // the sums in every lane
    double M[T], r[P];
    auto pass = [&](auto &&each) {
#pragma unroll
        for (int j = 0; j < T; ++j) M[j] = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) r[j] = 0.0;
        for (uint32_t i = lane; i < ns; i += 64u) {
            const double x = assoc_x(v, i, mode);
            if (x != x) continue;
            double xc[P];
            xc[0] = 1.0;
            xc[1] = x - mean[1];
#pragma unroll
            for (int j = 0; j < K; ++j) xc[2 + j] = a.cov[(uint64_t)j * ns + i] - mean[2 + j];
            double w, z;
            each(a.y[i], xc, w, z);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const double wx = w * xc[p];
                r[p] += wx * z;
#pragma unroll
                for (int q = 0; q <= p; ++q) M[tix(p, q)] += wx * xc[q];
            }
        }
#pragma unroll
        for (int j = 0; j < T; ++j) M[j] = wave_sum_f64(M[j]);
#pragma unroll
        for (int j = 0; j < P; ++j) r[j] = wave_sum_f64(r[j]);
    };
    // M, r -> beta and (M^-1)_xx; false: rank deficient
    auto solve = [&]() {
        double top = M[tix(0, 0)];
#pragma unroll
        for (int j = 1; j < P; ++j) top = M[tix(j, j)] > top ? M[tix(j, j)] : top;
        if (!cholesky<P>(M, kAssocRankTol * top)) return false;
        cholesky_solve<P>(M, r, beta);
        double e[P], col[P];
#pragma unroll
        for (int j = 0; j < P; ++j) e[j] = j == 1 ? 1.0 : 0.0;
        cholesky_solve<P>(M, e, col);
        inv_xx = col[1];
        return true;
    };
    auto eta_of = [&](const double (&xc)[P]) {
        double eta = beta[0];
#pragma unroll
        for (int j = 1; j < P; ++j) eta += beta[j] * xc[j];
        return eta;
    };

    if (BINARY) {
        double dev_old = 0.0, mu_min = 1.0;  // mu_min: the smallest min(mu, 1 - mu) of the last pass, this lane's samples
#pragma unroll 1
        for (int t = 0; t <= kAssocMaxIter; ++t) {
            // the deviance of iterate t (t = 0: of the start values) comes out of the same pass as the sums of step t + 1
            double dev = 0.0;
            mu_min = 1.0;
            pass([&](double y, const double (&xc)[P], double &w, double &z) {
                double eta, mu;
                if (t == 0) {
                    mu = (y + 0.5) * 0.5;
                    eta = log(mu / (1.0 - mu));
                } else {
                    eta = eta_of(xc);
                    mu = 1.0 / (1.0 + exp(-eta));
                    mu = mu < kAssocMuEps ? kAssocMuEps : mu > 1.0 - kAssocMuEps ? 1.0 - kAssocMuEps : mu;
                }
                dev += -2.0 * log(y != 0.0 ? mu : 1.0 - mu);
                const double tail = mu < 1.0 - mu ? mu : 1.0 - mu;
                mu_min = tail < mu_min ? tail : mu_min;
                w = mu * (1.0 - mu);
                z = eta + (y - mu) / w;
            });
            dev = wave_sum_f64(dev);
            if (t >= 1) {
                out.n_iter = (uint8_t)t;
                if (!(fabs(dev) < INFINITY)) {
                    out.status = INQ_ASSOC_ROW_NOT_CONVERGED;
                    break;
                }
                if (fabs(dev - dev_old) / (fabs(dev) + 0.1) < kAssocConverged) break;
                if (t == kAssocMaxIter) {
                    out.status = INQ_ASSOC_ROW_NOT_CONVERGED;
                    break;
                }
            }
            dev_old = dev;
            if (!solve()) {
                out.status = INQ_ASSOC_ROW_SINGULAR;
                break;
            }
        }
        if (out.status != INQ_ASSOC_ROW_SINGULAR) {
            out.beta = beta[1];
            out.se = sqrt(inv_xx);  // at the weights of the last weighted least squares, as glm.fit returns them
            out.stat = out.beta / out.se;
            out.p = erfc(fabs(out.stat) * 0.70710678118654752440);
        } else {
            out.n_iter = 0;
        }
        // the side output inq_assoc_rows_firth's fallback rule reads; rows stopped before the fit or SINGULAR ones leave it unread
        if (a.min_mu) {
            mu_min = wave_min_f64(mu_min);
            if (lane == 0) a.min_mu[row] = mu_min;
        }
    } else {
        pass([&](double y, const double (&)[P], double &w, double &z) { w = 1.0, z = y; });
        if (!solve()) {
            out.status = INQ_ASSOC_ROW_SINGULAR;
        } else {
            double rss = 0.0;
            for (uint32_t i = lane; i < ns; i += 64u) {
                const double x = assoc_x(v, i, mode);
                if (x != x) continue;
                double xc[P];
                xc[0] = 1.0;
                xc[1] = x - mean[1];
#pragma unroll
                for (int j = 0; j < K; ++j) xc[2 + j] = a.cov[(uint64_t)j * ns + i] - mean[2 + j];
                const double res = a.y[i] - eta_of(xc);
                rss += res * res;
            }
            rss = wave_sum_f64(rss);
            const uint32_t df = n - (uint32_t)P;  // >= 1 and <= n_samples
            out.beta = beta[1];
            out.se = sqrt(rss / (double)df * inv_xx);
            out.stat = out.beta / out.se;
            out.p = student_t_two_sided(out.stat, (double)df, a.tcoef[df]);
        }
    }
    if (lane == 0) a.rows[row] = out;
}

}  // namespace

void launch_assoc(const AssocArgs &a, hipStream_t s) {
    if (!a.n_rows) return;
    const dim3 grid((uint32_t)((a.n_rows + 3) / 4));
    assoc_for_p(a.k, [&](auto p_c) {
        constexpr int P = decltype(p_c)::value;
        if (a.outcome == INQ_ASSOC_BINARY) hipLaunchKernelGGL((assoc_kernel<P, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((assoc_kernel<P, false>), grid, dim3(256), 0, s, a);
    });
}

}  // namespace inq
