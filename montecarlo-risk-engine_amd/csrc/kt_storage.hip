// kt_storage.hip — forward-mode (tangent) kernels of the gas storage and of the model storages run on (include/mcx.h "K6 — gas
// storage", tangent block).  The dual images of k6_storage.hip's step and eval kernels, and dual paths of the Schwartz two-factor
// slot.
//
// The derivative (products/storage.py:219-308 of the reference): the three action values feed torch.argmax only, so NO gradient
// flows through the decision or through the continuation values used to take it.  Next state and volume change are functions of
// volumes: no parameter dependence.  The gradient flows through cash / numeraire of the chosen action (cash = -dv (spot +- cost),
// spot and numeraire dual atoms), through W_new[s] = cash_s / num + lerp(W_old, next state) with fixed weights, through the normal
// equations (host: G c = r => dc = G^-1 (dr - dG c)) into the coefficient tangents and from there into the exposure rows
// lerp_grid(c, state, x) / num with c, x, num dual and the state and its weights primal.
//
// Every PRIMAL value is formed by the functions k6_storage.hip forms it with (k6_common.h: the polynomial, the rate, the step
// candidate, the three candidates of an action date, one definition each), so image 0 equals the primal kernels' results by
// construction and every decision is the base run's; this file holds only what is dual.  The tangents are formed next to the
// primal values by hand and never feed a decision.  Decisions use the coefficients the caller passes (the base run's).
//   kts_step   one backward date.  One path per lane, the transition table and the coefficient rows are wave-uniform scalar loads.
//              The (1+NP)(2K-1) Gram sums stay in per-lane registers over the grid-stride loop and are reduced once at the end;
//              the (1+NP) S K right-hand-side moments cannot (640 at S = 32, K = 4): each is reduced over the wave as soon as it is
//              formed and lane 0 adds it to the wave's LDS row, as k6_step does for its one image (21.6 KB of LDS at K = 4).
//   kts_eval   the realised state of a path in a register (primal only), the cashflow and the exposure rows in dual numbers,
//              ADDED to the images mcx_tangent_eval has written.
//   kts_paths  Schwartz two-factor, EULER and ANALYTICAL: both step maps are linear in (x, y); the Cholesky factors depend on the
//              parameters (rho; under ANALYTICAL also kappa and the volatilities) and arrive with their tangents.
#include "mcx_dual.h"
#include "k6_common.h"

namespace {

constexpr int NP = MCX_TANGENT_NP;

// primal value exactly as dev_atom forms it, tangents by the chain rule: v = a + d x + b exp(c0 + c1 x)
struct KTSBook {
    const double* __restrict__ datoms;   // [n_atoms][5][NP]
    const double* __restrict__ paths;
    const double* __restrict__ dpaths;   // [NP][T][D][ld]
    int64_t ld, pstride, D;
};
__device__ __forceinline__ void kts_atom(const KTSBook& b, const DevAtom& a, int id, int64_t i, double& v, double (&dv)[NP])
{
    const double* __restrict__ da = b.datoms + (int64_t)id * 5 * NP;
    double x = 0.0, dx[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) dx[q] = 0.0;
    if (a.col >= 0) {
        const int64_t off = ((int64_t)a.t_idx * b.D + a.col) * b.ld + i;
        x = b.paths[off];
#pragma unroll
        for (int q = 0; q < NP; ++q) dx[q] = b.dpaths[q * b.pstride + off];
    }
    v = fma(a.d, x, a.a);
#pragma unroll
    for (int q = 0; q < NP; ++q) dv[q] = ldk(da + q) + ldk(da + NP + q) * x + a.d * dx[q];
    if (a.b != 0.0) {
        const double E = mcx_exp(fma(a.c1, x, a.c0));
        v = fma(a.b, E, v);
        const double bE = a.b * E;
#pragma unroll
        for (int q = 0; q < NP; ++q) dv[q] += ldk(da + 2 * NP + q) * E + bE * (ldk(da + 3 * NP + q) + ldk(da + 4 * NP + q) * x + a.c1 * dx[q]);
    }
}

// ---- backward step -----------------------------------------------------------------------------------------------------------
struct KTSStepArgs {
    KTSBook b;
    const double* __restrict__ W_old;
    const double* __restrict__ dW_old;     // [NP][S][ld_w]
    double* __restrict__ W_new;
    double* __restrict__ dW_new;
    double* __restrict__ partials;         // [gridDim.x][1+NP][NM]
    const double* __restrict__ coeffs;     // [S][K] block of the rolled date in the array the decisions are taken from
    const double* __restrict__ trans;      // [S][3][2] of the rolled date
    KTSAtom num, x, rnum, rx;
    double shift, scale, c_inj, c_wd;
    int64_t n, ld_w, w_stride;             // w_stride = S * ld_w (between tangents)
    int32_t S, roll, is_last, f32_cache;
};

template <int K>
__global__ __launch_bounds__(MCX_BLOCK) void kts_step(const KTSStepArgs a)
{
    constexpr int NB = 2 * K - 1, ROW = NB + K6_MAX_S * K;
    __shared__ double rows[4][1 + NP][ROW];
    const int NM = NB + a.S * K;
    const int lane = threadIdx.x & (MCX_WAVE - 1), wv = threadIdx.x >> 6;
    for (int q = lane; q < (1 + NP) * ROW; q += MCX_WAVE) (&rows[wv][0][0])[q] = 0.0;     // (each wave owns its rows)
    double gram[1 + NP][NB];
#pragma unroll
    for (int q = 0; q <= NP; ++q)
#pragma unroll
        for (int k = 0; k < NB; ++k) gram[q][k] = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * MCX_BLOCK; base < a.n; base += (int64_t)gridDim.x * MCX_BLOCK) {
        const int64_t i_raw = base + threadIdx.x;
        const bool live = i_raw < a.n;
        const int64_t i = live ? i_raw : a.n - 1;                       // idle lanes read a valid path and contribute zero
        double num, dnum[NP], xv, dxv[NP];
        kts_atom(a.b, a.num.a, a.num.id, i, num, dnum);
        kts_atom(a.b, a.x.a, a.x.id, i, xv, dxv);
        const double z = (xv - a.shift) * a.scale;
        double dz[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) dz[q] = dxv[q] * a.scale;
        {
            double zp = 1.0, dzp[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) dzp[q] = 0.0;
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                if (live) {
                    gram[0][k] += zp;
#pragma unroll
                    for (int q = 0; q < NP; ++q) gram[1 + q][k] += dzp[q];
                }
#pragma unroll
                for (int q = 0; q < NP; ++q) dzp[q] = dzp[q] * z + zp * dz[q];
                zp *= z;
            }
        }
        double spot = 0.0, rnum = 1.0, dspot[NP], drnum[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) dspot[q] = drnum[q] = 0.0;
        if (a.roll) { kts_atom(a.b, a.rx.a, a.rx.id, i, spot, dspot); kts_atom(a.b, a.rnum.a, a.rnum.id, i, rnum, drnum); }
        const double p_inj = spot + a.c_inj, p_wd = spot - a.c_wd;
        for (int s = 0; s < a.S; ++s) {
            double w, dw[NP];
            if (a.roll) {
                const double* __restrict__ t = a.trans + s * 6;
                const double ns0 = ldk(t + 0), dv0 = ldk(t + 1), ns1 = ldk(t + 2), dv1 = ldk(t + 3), ns2 = ldk(t + 4), dv2 = ldk(t + 5);
                double c0, v0, t0, c1, v1, t1, c2, v2, t2, f0, f1, f2;
                int lo0, hi0, lo1, hi1, lo2, hi2;
                k6_step_candidate<K>(a.coeffs, a.W_old, a.ld_w, a.S, a.is_last, ns0, dv0, p_inj, spot, i, c0, v0, t0, lo0, hi0, f0);                      // inject
                k6_step_candidate<K>(a.coeffs, a.W_old, a.ld_w, a.S, a.is_last, ns1, dv1, dv1 >= 0.0 ? p_inj : p_wd, spot, i, c1, v1, t1, lo1, hi1, f1);  // hold
                k6_step_candidate<K>(a.coeffs, a.W_old, a.ld_w, a.S, a.is_last, ns2, dv2, p_wd, spot, i, c2, v2, t2, lo2, hi2, f2);                      // withdraw
                const bool m1 = v1 > v0;                                   // the first maximum wins (torch.argmax)
                const double vb1 = m1 ? v1 : v0;
                const bool m2 = v2 > vb1;
                const double cb = m2 ? c2 : (m1 ? c1 : c0), tb = m2 ? t2 : (m1 ? t1 : t0), dvb = m2 ? dv2 : (m1 ? dv1 : dv0);
                const double fb = m2 ? f2 : (m1 ? f1 : f0);
                const int lob = m2 ? lo2 : (m1 ? lo1 : lo0), hib = m2 ? hi2 : (m1 ? hi1 : hi0);
                double c = cb / rnum;
                const double ir = 1.0 / rnum;
#pragma unroll
                for (int q = 0; q < NP; ++q) {                             // d(cash / num) + the tail's tangent at the fixed weights
                    const double t_lo = a.dW_old[q * a.w_stride + (int64_t)lob * a.ld_w + i];
                    const double t_hi = hib != lob ? a.dW_old[q * a.w_stride + (int64_t)hib * a.ld_w + i] : t_lo;
                    dw[q] = (-dvb * dspot[q] - c * drnum[q]) * ir + (t_lo + fb * (t_hi - t_lo));
                }
                if (a.f32_cache) c = (double)(float)c;                     // the primal cash term only (float32 step buffer of the base run)
                w = c + tb;
                if (live) {
                    a.W_new[(int64_t)s * a.ld_w + i] = w;
#pragma unroll
                    for (int q = 0; q < NP; ++q) a.dW_new[q * a.w_stride + (int64_t)s * a.ld_w + i] = dw[q];
                }
            } else {
                w = a.W_old[(int64_t)s * a.ld_w + i];
#pragma unroll
                for (int q = 0; q < NP; ++q) dw[q] = a.dW_old[q * a.w_stride + (int64_t)s * a.ld_w + i];
            }
            const double y = num * w;
            double dy[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) dy[q] = dnum[q] * w + num * dw[q];
            double zp = 1.0, dzp[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) dzp[q] = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double r = wave_sum(live ? zp * y : 0.0);
                if (lane == 0) rows[wv][0][NB + s * K + k] += r;
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const double rq = wave_sum(live ? dzp[q] * y + zp * dy[q] : 0.0);
                    if (lane == 0) rows[wv][1 + q][NB + s * K + k] += rq;
                }
#pragma unroll
                for (int q = 0; q < NP; ++q) dzp[q] = dzp[q] * z + zp * dz[q];
                zp *= z;
            }
        }
    }
#pragma unroll
    for (int q = 0; q <= NP; ++q)
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const double r = wave_sum(gram[q][k]);
            if (lane == 0) rows[wv][q][k] = r;
        }
    __syncthreads();
    for (int e = threadIdx.x; e < (1 + NP) * NM; e += MCX_BLOCK) {
        const int q = e / NM, m = e - q * NM;
        a.partials[(int64_t)blockIdx.x * (1 + NP) * NM + e] = (rows[0][q][m] + rows[1][q][m]) + (rows[2][q][m] + rows[3][q][m]);
    }
}

// ---- main simulation ---------------------------------------------------------------------------------------------------------
struct KTSEvalArgs {
    KTSBook b;
    const KTSDate* __restrict__ dates;
    const mcx_storage_op* __restrict__ ops;
    const DevAtom* __restrict__ atoms;
    const double* __restrict__ coeffs;     // [n_coeffs]: decisions and exposure values
    const double* __restrict__ dcoeffs;    // [n_coeffs][NP]
    double* __restrict__ cfs;              // the netting set's row of image 0
    double* __restrict__ expo;             // the netting set's [n_rows][ld_out] block of image 0
    int64_t n, ld_out, cf_stride, ex_stride;
    int32_t n_ops, S;
};

// tangent of the polynomial row c (dual) at x (dual): sum_k dc_k x^k + (sum_k k c_k x^(k-1)) dx
template <int K>
__device__ __forceinline__ void kts_dpoly(const double* __restrict__ c, const double* __restrict__ dc, double x, const double (&dx)[NP], double (&out)[NP])
{
    double gx = 0.0, xp = 1.0, acc[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) acc[q] = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int q = 0; q < NP; ++q) acc[q] = fma(dc[k * NP + q], xp, acc[q]);
        if (k + 1 < K) gx = fma((double)(k + 1) * c[k + 1], xp, gx);
        xp *= x;
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) out[q] = acc[q] + gx * dx[q];
}

template <int K>
__global__ __launch_bounds__(MCX_BLOCK) void kts_eval(const KTSEvalArgs a)
{
    __shared__ KTSDate sd;
    __shared__ double sc[K6_MAX_S * K];
    __shared__ double sdc[K6_MAX_S * K * NP];
    const int64_t i_raw = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    const bool live = i_raw < a.n;
    const int64_t i = live ? i_raw : a.n - 1;
    double state = 0.0, cf = 0.0, dcf[NP];                              // get_initial_state() = 0.0
#pragma unroll
    for (int q = 0; q < NP; ++q) dcf[q] = 0.0;
    for (int op = 0; op < a.n_ops; ++op) {
        const mcx_storage_op o = ldk_struct(a.ops + op);
        __syncthreads();                                                // the previous op's readers are done with sd / sc / sdc
        int64_t off = o.coeff_off;
        bool need_coeffs = true;
        if (o.kind == 0) {
            const uint32_t* __restrict__ src = (const uint32_t*)(a.dates + o.index);
            for (int q = threadIdx.x; q < (int)(sizeof(KTSDate) / 4); q += MCX_BLOCK) ((uint32_t*)&sd)[q] = src[q];
            off = ldk(&a.dates[o.index].coeff_off);
            need_coeffs = ldk(&a.dates[o.index].is_last) == 0;
        }
        if (need_coeffs) {
            for (int q = threadIdx.x; q < a.S * K; q += MCX_BLOCK) sc[q] = a.coeffs[off + q];
            if (o.kind != 0)
                for (int q = threadIdx.x; q < a.S * K * NP; q += MCX_BLOCK) sdc[q] = a.dcoeffs[off * NP + q];
        }
        __syncthreads();
        if (o.kind == 0) {
            double spot, num, dspot[NP], dnum[NP];
            kts_atom(a.b, sd.x.a, sd.x.id, i, spot, dspot);
            kts_atom(a.b, sd.num.a, sd.num.id, i, num, dnum);
            K6Cand c0, c1, c2;                                          // inject, hold, withdraw
            const double v = k6_eval_candidates<K>(sd, sc, a.S, state, spot, c0, c1, c2);
            const bool m1 = c1.value > c0.value;                        // the first maximum wins (torch.argmax); selects: no scratch
            const double vb1 = m1 ? c1.value : c0.value;
            const bool m2 = c2.value > vb1;
            const double cb = m2 ? c2.cash : (m1 ? c1.cash : c0.cash), nvb = m2 ? c2.nv : (m1 ? c1.nv : c0.nv);
            state = m2 ? c2.ns : (m1 ? c1.ns : c0.ns);
            const double cn = cb / num, ir = 1.0 / num, mdv = -(nvb - v);
            cf += cn;
#pragma unroll
            for (int q = 0; q < NP; ++q) dcf[q] += (mdv * dspot[q] - cn * dnum[q]) * ir;
        } else {
            const DevAtom an = ldk_struct(a.atoms + o.num_atom), ax = ldk_struct(a.atoms + o.x_atom);
            double x, num, dx[NP], dnum[NP];
            kts_atom(a.b, ax, o.x_atom, i, x, dx);
            kts_atom(a.b, an, o.num_atom, i, num, dnum);
            const double e = k6_lerp_grid<K>(sc, a.S, state, x) / num;
            const double b = fmin(fmax(state, 0.0), (double)(a.S - 1));
            const double fl = floor(b), w = b - fl;
            const int lo = (int)fl, hi = (int)ceil(b);
            double d_lo[NP], d_hi[NP];
            kts_dpoly<K>(sc + lo * K, sdc + lo * K * NP, x, dx, d_lo);
            kts_dpoly<K>(sc + hi * K, sdc + hi * K * NP, x, dx, d_hi);
            const double ir = 1.0 / num;
            if (live) {
                const int64_t eo = (int64_t)o.index * a.ld_out + i;
                a.expo[eo] += e;
#pragma unroll
                for (int q = 0; q < NP; ++q) a.expo[(1 + q) * a.ex_stride + eo] += ((d_lo[q] + w * (d_hi[q] - d_lo[q])) - e * dnum[q]) * ir;
            }
        }
    }
    if (live) {
        a.cfs[i] += cf;
#pragma unroll
        for (int q = 0; q < NP; ++q) a.cfs[(1 + q) * a.cf_stride + i] += dcf[q];
    }
}

// ---- Schwartz two-factor dual paths ----------------------------------------------------------------------------------------------
struct KTSPathArgs {
    K1Args k1;
    const double* __restrict__ dslot;   // [MCX_SLOT_NPARAM][NP]
    const double* __restrict__ dinit;   // [3][NP]
    const double* __restrict__ daux;    // [n_steps][MCX_AUX][NP]
    const double* __restrict__ dchol;   // [n_chol][2][2][NP]
    double* __restrict__ dpaths;        // [NP][T][3][ld]
    int64_t pstride;
};

__device__ __forceinline__ void kts_write_state(const KTSPathArgs& a, int t, int64_t i, double logF, const double* __restrict__ dlogF,
                                                double x, const double (&dx)[NP], double y, const double (&dy)[NP])
{
    const K1Args& k = a.k1;
    const int64_t off = (int64_t)t * 3 * k.ld + i;
    k.paths[off] = (logF + x) + y;                       // sim_store_state: log S = log F0(t) + x + y
    k.paths[off + k.ld] = x;
    k.paths[off + 2 * k.ld] = y;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        double* __restrict__ dp = a.dpaths + q * a.pstride + off;
        dp[0] = (ldk(dlogF + q) + dx[q]) + dy[q];
        dp[k.ld] = dx[q];
        dp[2 * k.ld] = dy[q];
    }
}

template <bool INJECT>
__global__ __launch_bounds__(MCX_BLOCK) void kts_paths(const KTSPathArgs a)
{
    const K1Args& k = a.k1;
    __shared__ double bm_lds[INJECT ? 2 : MCX_BM_LDS_DOUBLES];
    const double* tab = nullptr;
    if (!INJECT) { mcx_bm_load(bm_lds); tab = bm_lds; }
    const int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    if (i >= k.n) return;
    const double* __restrict__ p = k.slots[0].p;
    double x = k.init_state[1], y = k.init_state[2], dx[NP], dy[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) { dx[q] = ldk(a.dinit + NP + q); dy[q] = ldk(a.dinit + 2 * NP + q); }
    for (int t = 0; t < k.n_initial_store; ++t) kts_write_state(a, t, i, p[6], a.dslot + 6 * NP, x, dx, y, dy);
    const uint64_t path = k.path_offset + (uint64_t)i;
    const bool analytical = k.scheme == MCX_SCHEME_ANALYTICAL;
#pragma unroll 1
    for (int step = 0; step < k.n_steps; ++step) {
        const mcx_step sp = ldk_struct(&k.steps[step]);
        double z0, z1;
        if (INJECT) {
            z0 = k.inject_z[((int64_t)step * 2 + 0) * k.ld + i];
            z1 = k.inject_z[((int64_t)step * 2 + 1) * k.ld + i];
        } else {
            double ua;
            draw_pair<true>(k.seed, path, (uint32_t)step, 0u, ua, z0, z1, tab);
        }
        // sim_apply: the one factor of the correlation matrix under EULER (its first entry is exactly 1), one per distinct dt otherwise
        const int ci = analytical ? sp.chol_idx : 0;
        const double* __restrict__ L = k.chol + (int64_t)ci * 4;
        const double* __restrict__ dL = a.dchol + (int64_t)ci * 4 * NP;
        const double zc0 = analytical ? ldk(L + 0) * z0 : z0;
        const double zc1 = fma(ldk(L + 3), z1, ldk(L + 2) * z0);
        const double* __restrict__ ax = k.aux + (int64_t)step * MCX_AUX;
        const double* __restrict__ dax = a.daux + (int64_t)step * MCX_AUX * NP;
        const double dt = sp.dt, sq = sp.sqrt_dt;
        const double x0 = x, y0 = y;
        if (analytical) {                                                 // step_slot, MCX_MODEL_S2F
            const double decay = ldk(ax + 0);
            x = x0 * decay + zc0;
            y = y0 + p[3] * dt + zc1;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                dx[q] = dx[q] * decay + x0 * ldk(dax + q) + ldk(dL + q) * z0;
                dy[q] = dy[q] + ldk(a.dslot + 3 * NP + q) * dt + (ldk(dL + 2 * NP + q) * z0 + ldk(dL + 3 * NP + q) * z1);
            }
        } else {
            x = x0 - p[1] * x0 * dt + p[2] * sq * zc0;
            y = y0 + p[3] * dt + p[4] * sq * zc1;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const double dzc0 = ldk(dL + q) * z0, dzc1 = ldk(dL + 2 * NP + q) * z0 + ldk(dL + 3 * NP + q) * z1;
                dx[q] = dx[q] - (ldk(a.dslot + 1 * NP + q) * x0 + p[1] * dx[q]) * dt + (ldk(a.dslot + 2 * NP + q) * zc0 + p[2] * dzc0) * sq;
                dy[q] = dy[q] + ldk(a.dslot + 3 * NP + q) * dt + (ldk(a.dslot + 4 * NP + q) * zc1 + p[4] * dzc1) * sq;
            }
        }
        if (sp.store_idx >= 0) kts_write_state(a, sp.store_idx, i, ldk(ax + 1), dax + NP, x, dx, y, dy);
    }
}

void kts_fill_book(const mcx_book* b, const double* d_datoms, const double* d_paths, const double* d_dpaths, int64_t ld, int32_t n_dates,
                   KTSBook* out)
{
    out->datoms = d_datoms; out->paths = d_paths; out->dpaths = d_dpaths; out->ld = ld; out->D = b->n_state;
    out->pstride = (int64_t)n_dates * b->n_state * ld;
}

// the shared descriptor checks and the tangent kernels' own bound on the basis size
int kts_check_desc(mcx_handle* h, const mcx_book* b, const mcx_storage_desc* d, const char* who)
{
    if (int rc = k6_check_desc(h, b, d, who)) return rc;
    if (b->n_basis < 1 || b->n_basis > 4) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: basis size %d has no instantiation", who, b->n_basis);
    return 0;
}

}  // namespace

extern "C" int mcx_tangent_storage_lsm_step(mcx_handle* h, const mcx_book* b, const mcx_storage_desc* desc, int32_t roll_date, int32_t num_atom,
                                            int32_t x_atom, double shift, double scale, const double* d_datoms, const double* d_coeffs,
                                            const double* d_paths, const double* d_dpaths, int64_t n_paths, int64_t ld, int32_t n_dates,
                                            const double* d_W_old, const double* d_dW_old, double* d_W_new, double* d_dW_new, int64_t ld_w,
                                            double* h_moments, int32_t flags, void* stream)
{
    const char* who = "mcx_tangent_storage_lsm_step";
    if (!h || !b || !desc || !d_datoms || !d_coeffs || !d_paths || !d_dpaths || !d_W_old || !d_dW_old || !h_moments) return -1;
    if (int rc = kts_check_desc(h, b, desc, who)) return rc;
    if (roll_date >= desc->n_dates) MCX_FAIL(h, -2, "%s: roll date out of range", who);
    if (roll_date >= 0) if (int rc = k6_check_date(h, b, desc, roll_date, who)) return rc;
    if (num_atom < 0 || num_atom >= b->n_atoms || x_atom < 0 || x_atom >= b->n_atoms) MCX_FAIL(h, -2, "%s: atom out of range", who);
    if (ld < n_paths || ld_w < n_paths) MCX_FAIL(h, -2, "%s: leading dimension < n_paths", who);
    if (roll_date >= 0 && (!d_W_new || !d_dW_new || d_W_new == d_W_old || d_dW_new == d_dW_old))
        MCX_FAIL(h, -2, "%s: a roll needs a second pair of cache buffers", who);
    const int K = b->n_basis, S = desc->n_states, NM = (2 * K - 1) + S * K, count = (1 + NP) * NM;
    if (n_paths <= 0) { memset(h_moments, 0, sizeof(double) * (size_t)count); return 0; }
    hipStream_t s = (hipStream_t)stream;
    const int grid = mcx_grid_for(n_paths, MCX_BLOCK, 4 * h->n_cu);
    KTSStepArgs a;
    memset(&a, 0, sizeof(a));
    kts_fill_book(b, d_datoms, d_paths, d_dpaths, ld, n_dates, &a.b);
    a.W_old = d_W_old; a.dW_old = d_dW_old; a.W_new = d_W_new; a.dW_new = d_dW_new;
    if (!(a.partials = mcx_partials_ws(h, who, grid, count))) return -2;
    k6_set_atom(b, num_atom, a.num); k6_set_atom(b, x_atom, a.x); a.rnum = a.num; a.rx = a.x;
    a.shift = shift; a.scale = scale; a.n = n_paths; a.ld_w = ld_w; a.w_stride = (int64_t)S * ld_w; a.S = S;
    a.f32_cache = (flags & MCX_LSM_F32_CACHE) ? 1 : 0;
    a.roll = roll_date >= 0; a.is_last = 1; a.coeffs = d_coeffs; a.trans = nullptr;
    if (a.roll) {
        const mcx_storage_date& d = desc->dates[roll_date];
        const double* d_trans = (const double*)mcx_stage_small(h, desc->trans + (size_t)roll_date * S * 6, sizeof(double) * (size_t)S * 6, s);
        if (!d_trans) return -100;
        a.coeffs = d_coeffs + d.coeff_off; a.trans = d_trans;
        k6_set_atom(b, d.num_atom, a.rnum); k6_set_atom(b, d.x_atom, a.rx); a.c_inj = d.c_inj; a.c_wd = d.c_wd; a.is_last = d.is_last ? 1 : 0;
    }
    K6_DISPATCH(K, 4, hipLaunchKernelGGL((kts_step<KK>), dim3(grid), dim3(MCX_BLOCK), 0, s, a));
    MCX_HIP(h, hipGetLastError());
    return mcx_partials_to_host(h, grid, count, h_moments, s);
}

extern "C" int mcx_tangent_storage_eval(mcx_handle* h, const mcx_book* b, const mcx_storage_desc* desc, const mcx_storage_op* h_ops, int32_t n_ops,
                                        const double* d_datoms, const double* d_coeffs, const double* d_dcoeffs, const double* d_paths,
                                        const double* d_dpaths, int64_t n_paths, int64_t ld, int32_t n_dates, double* d_cfs, double* d_expo,
                                        int64_t ld_out, void* stream)
{
    const char* who = "mcx_tangent_storage_eval";
    if (!h || !b || !desc || !h_ops || !d_datoms || !d_coeffs || !d_dcoeffs || !d_paths || !d_dpaths || !d_cfs || !d_expo) return -1;
    if (n_paths <= 0 || n_ops <= 0) return 0;
    if (int rc = kts_check_desc(h, b, desc, who)) return rc;
    if (ld < n_paths || ld_out < n_paths) MCX_FAIL(h, -2, "%s: leading dimension < n_paths", who);
    const int K = b->n_basis, S = desc->n_states;
    const int n_rows = b->n_expo_rows > 0 ? b->n_expo_rows : 1;
    for (int q = 0; q < n_ops; ++q) {
        const mcx_storage_op& o = h_ops[q];
        if (o.kind == 0) {
            if (o.index < 0 || o.index >= desc->n_dates) MCX_FAIL(h, -2, "%s: op %d: action date out of range", who, q);
        } else if (o.kind == 1) {
            if (o.index < 0 || o.index >= b->n_expo_rows) MCX_FAIL(h, -2, "%s: op %d: exposure row out of range", who, q);
            if (o.num_atom < 0 || o.num_atom >= b->n_atoms || o.x_atom < 0 || o.x_atom >= b->n_atoms) MCX_FAIL(h, -2, "%s: op %d: atom out of range", who, q);
            if (o.coeff_off < 0 || o.coeff_off + (int64_t)S * K > b->n_coeffs) MCX_FAIL(h, -2, "%s: op %d: coefficient block out of range", who, q);
        } else MCX_FAIL(h, -2, "%s: op %d: bad kind", who, q);
    }
    std::vector<KTSDate> dates((size_t)desc->n_dates);
    for (int j = 0; j < desc->n_dates; ++j) {
        if (int rc = k6_check_date(h, b, desc, j, who)) return rc;
        k6_fill_date(b, desc->dates[j], dates[j]);
    }
    hipStream_t s = (hipStream_t)stream;
    const void* d_dates = mcx_upload_table(h, 0, dates.data(), sizeof(KTSDate) * dates.size(), s);
    const void* d_ops = mcx_upload_table(h, 1, h_ops, sizeof(mcx_storage_op) * (size_t)n_ops, s);
    if (!d_dates || !d_ops) return -100;
    KTSEvalArgs a;
    memset(&a, 0, sizeof(a));
    kts_fill_book(b, d_datoms, d_paths, d_dpaths, ld, n_dates, &a.b);
    a.dates = (const KTSDate*)d_dates; a.ops = (const mcx_storage_op*)d_ops; a.atoms = b->d_atoms;
    a.coeffs = d_coeffs; a.dcoeffs = d_dcoeffs;
    a.cfs = d_cfs + (size_t)desc->netting_set * ld_out;
    a.expo = d_expo + (size_t)desc->netting_set * n_rows * ld_out;
    a.cf_stride = (int64_t)b->n_netting_sets * ld_out; a.ex_stride = (int64_t)b->n_netting_sets * n_rows * ld_out;
    a.n = n_paths; a.ld_out = ld_out; a.n_ops = n_ops; a.S = S;
    const int grid = (int)((n_paths + MCX_BLOCK - 1) / MCX_BLOCK);
    K6_DISPATCH(K, 4, hipLaunchKernelGGL((kts_eval<KK>), dim3(grid), dim3(MCX_BLOCK), 0, s, a));
    MCX_HIP(h, hipGetLastError());
    MCX_HIP(h, hipStreamSynchronize(s));
    return 0;
}

extern "C" int mcx_tangent_paths_s2f(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux,
                                     const double* h_dchol, uint64_t seed, uint64_t path_offset, int64_t n_paths, double* d_paths,
                                     double* d_dpaths, int64_t ld, const double* d_inject_z, void* stream)
{
    const char* who = "mcx_tangent_paths_s2f";
    if (!h_dchol) return -1;                              // (read under both schemes)
    if (int rc = mcx_tangent_check_args(h, sim, h_dslot, h_dinit, h_daux, h_dchol, 0u, d_paths, d_dpaths, n_paths, ld, who, false, who))
        return rc > 0 ? 0 : rc;
    const mcx_sim_desc& sd = sim->desc;
    if (sd.n_slots != 1 || sd.slots[0].kind != MCX_MODEL_S2F || sd.n_z != 2 || sd.n_state != 3)
        MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: a single Schwartz two-factor slot expected", who);
    if (sd.scheme != MCX_SCHEME_EULER && sd.scheme != MCX_SCHEME_ANALYTICAL) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: EULER or ANALYTICAL scheme", who);
    if (int rc = mcx_tangent_check_steps(h, who, sim, sd.n_chol, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    mcx_tangent_tables t;
    if (int rc = mcx_tangent_upload(h, sd, h_dslot, h_dinit, h_daux, h_dchol, s, &t)) return rc;
    KTSPathArgs a;
    memset(&a, 0, sizeof(a));
    mcx_fill_k1_args(sim, seed, path_offset, n_paths, ld, d_paths, d_inject_z, nullptr, &a.k1);
    a.dslot = t.dslot; a.dinit = t.dinit; a.daux = t.daux; a.dchol = t.dchol;
    a.dpaths = d_dpaths; a.pstride = (int64_t)sd.n_dates * 3 * ld;
    const int grid = (int)((n_paths + MCX_BLOCK - 1) / MCX_BLOCK);
    if (d_inject_z) hipLaunchKernelGGL((kts_paths<true>), dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((kts_paths<false>), dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    MCX_HIP(h, hipGetLastError());
    MCX_HIP(h, hipStreamSynchronize(s));
    return 0;
}
