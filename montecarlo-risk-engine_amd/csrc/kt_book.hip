// kt_book.hip — forward-mode (tangent) pass through the WHOLE exposure path: paths, LSM regression, book evaluation, CVA.
//
// The reference obtains d CVA / d theta by taping pre-simulation + lstsq + main simulation and calling torch.autograd.grad
// (controller/controller.py:609-627, regression coefficients carry their graph: :370-383).  Here the derivative travels
// forward in dual numbers, MCX_TANGENT_NP parameters per pass:
//   kt_paths : K1 with dual state           -> paths [T][D][N] and d paths / d theta [NP][T][D][N]
//   kt_lsm_batch : normal equations of (product, regression date) jobs with dual moments (the host differentiates the solve:
//              G c = r  =>  dc = G^-1 (dr - dG c)); mcx_tangent_lsm is its one-job case
//   kt_eval  : the book's cashflow / polynomial-exposure events with dual atoms and dual coefficients
//   kt_cva   : sum_m relu(thr(E_m)) S(0,t_m) (1 - S(t_m,t_m+1)) (1-R) per path with tangents (cva_metric.py:62-100)
//   kt_xva   : the five bilateral xVA records (cva, dva, their first-to-default forms, bcva) with tangents, summed over the paths in
//              the same launch (the dual of k4_xva.hip; mcx/metrics/bcva_metric.py)
// The derivatives of every host-computed descriptor number (model parameters per slot, psi(t) tables, initial state, the
// closed-form coefficients of each atom) arrive as arrays next to the primal descriptors (mcx/aad.py builds them).
//   kt_lsm_step : the same for products with exercise rights (Bermudan / American / FlexiCall): the cashflow cache rolled back
//              along the FROZEN exercise policy in dual numbers, moments per hypothetical state
// Scope: EULER scheme with Black-Scholes / Vasicek / CIR++ (stochastic and deterministic) slots, ANALYTICAL scheme with Black-Scholes /
// Vasicek slots (mcx_tangent_paths_chol: the Cholesky factor of the per-dt covariance carries a tangent), a single Heston slot under
// EULER or QE (mcx_tangent_paths_heston); cashflow, plain option and
// exercise events, polynomial (also state-indexed) and analytic Black-Scholes exposures; thresholds and MPoR collateral in the
// metric kernels; option events in the payoff modes 1-5 (geometric, control variate, binary, barrier, bridge) in kt_eval and
// kt_lsm_batch while the book is armed (mcx_book_set_payoff_tangents).  Anything else keeps the common-random-number bump path.
#include <stdlib.h>

#include <algorithm>

#include "mcx_dual_step.h"

namespace {

// ---- paths -------------------------------------------------------------------------------------------------------------
struct KTPArgs {
    K1Args k1;
    const double* __restrict__ dslot;   // [n_slots][MCX_SLOT_NPARAM][NP]
    const double* __restrict__ dinit;   // [n_state][NP]
    const double* __restrict__ daux;    // [n_steps][n_slots][MCX_AUX][NP]
    double* __restrict__ dpaths;        // [NP][T][D][ld]
    int64_t pstride;                    // T * D * ld
    int32_t n_slots, pad;
};

template <int NSLOT>
__device__ __forceinline__ void ktp_store(const KTPArgs& a, int t, int64_t i, const DN (&reg)[2 * NSLOT])
{
    const K1Args& k = a.k1;
    const int D = k.n_state;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        const int c = k.slots[s].state_off;
        const int nd = k.slots[s].kind == MCX_MODEL_BS ? 1 : 2;
        for (int e = 0; e < nd; ++e) {
            dstore(k.paths, a.dpaths, a.pstride, ((int64_t)t * D + c + e) * k.ld + i, reg[2 * s + e]);
        }
    }
}

template <int NSLOT, int NZ, bool INJECT>
__global__ __launch_bounds__(MCX_BLOCK) void kt_paths(const KTPArgs a)
{
    const K1Args& k = a.k1;
    __shared__ double bm_lds[INJECT ? 2 : MCX_BM_LDS_DOUBLES];
    const double* tab = nullptr;
    if (!INJECT) { mcx_bm_load(bm_lds); tab = bm_lds; }
    const int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    if (i >= k.n) return;
    DN reg[2 * NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        const int c = k.slots[s].state_off;
        const bool bs = k.slots[s].kind == MCX_MODEL_BS;
        reg[2 * s] = ld_dual(k.init_state[c], a.dinit + (int64_t)c * NP);
        reg[2 * s + 1] = bs ? dconst<NP>(0.0) : ld_dual(k.init_state[c + 1], a.dinit + (int64_t)(c + 1) * NP);
    }
    for (int t = 0; t < k.n_initial_store; ++t) ktp_store<NSLOT>(a, t, i, reg);
    const uint64_t path = k.path_offset + (uint64_t)i;
#pragma unroll 1
    for (int step = 0; step < k.n_steps; ++step) {
        const mcx_step sp = ldk_struct(&k.steps[step]);
        double z[NZ], zc[NZ];
        if (INJECT) {
#pragma unroll
            for (int j = 0; j < NZ; ++j) z[j] = k.inject_z[((int64_t)step * NZ + j) * k.ld + i];
        } else {
#pragma unroll
            for (int q = 0; q < (NZ + 1) / 2; ++q) {
                double ua, z0, z1;
                draw_pair<true>(k.seed, path, (uint32_t)step, (uint32_t)q, ua, z0, z1, tab);
                z[2 * q] = z0;
                if (2 * q + 1 < NZ) z[2 * q + 1] = z1;
            }
        }
        const double* __restrict__ L = k.chol + (int64_t)sp.chol_idx * NZ * NZ;
#pragma unroll
        for (int r = 0; r < NZ; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c <= r; ++c) acc += ldk(L + r * NZ + c) * z[c];
            zc[r] = acc;
        }
        const double dt = sp.dt, sq = sp.sqrt_dt;
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            const DualKarg p{k.slots[s].p, a.dslot + (int64_t)s * MCX_SLOT_NPARAM * NP};
            const DualTable ax{k.aux + ((int64_t)step * NSLOT + s) * MCX_AUX, a.daux + ((int64_t)step * NSLOT + s) * MCX_AUX * NP};
            dual_step_euler<false>(k.slots[s].kind, p, ax, dt, sq, zc[s < NZ ? s : 0], reg[2 * s], reg[2 * s + 1]);
        }
        const int st = sp.store_idx;
        if (st >= 0) ktp_store<NSLOT>(a, st, i, reg);
    }
}

// kt_paths in its second mode: the ANALYTICAL scheme of Black-Scholes and Vasicek slots, one normal per slot.  The factor of the
// per-dt covariance depends on the parameters: row s of it is a dual number (dchol next to k.chol, both wave-uniform), and the step
// maps are the primal analytic branches of step_slot (mcx_device.h) in dual numbers (dual_step_analytical of mcx_dual_step.h, next to
// kt_paths' dual_step_euler).  Initial state, draws (the same normals as the EULER mode and as K1: one Box-Muller pair per two, an odd
// NZ drops the last sine) and stores as kt_paths.  Those two loops are written out in both kernels on purpose: as one shared function
// the initial-state loop changed the compiled code of all 16 instantiations of the two kernels, the draw loop that of 10.
struct KTPCholArgs {
    KTPArgs p;
    const double* __restrict__ dchol;   // [n_chol][n_z][n_z][NP]
};

template <int NSLOT, int NZ, bool INJECT>
__global__ __launch_bounds__(MCX_BLOCK) void kt_paths_chol(const KTPCholArgs ca)
{
    const KTPArgs& a = ca.p;
    const K1Args& k = a.k1;
    __shared__ double bm_lds[INJECT ? 2 : MCX_BM_LDS_DOUBLES];
    const double* tab = nullptr;
    if (!INJECT) { mcx_bm_load(bm_lds); tab = bm_lds; }
    const int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    if (i >= k.n) return;
    DN reg[2 * NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        const int c = k.slots[s].state_off;
        const bool bs = k.slots[s].kind == MCX_MODEL_BS;
        reg[2 * s] = ld_dual(k.init_state[c], a.dinit + (int64_t)c * NP);
        reg[2 * s + 1] = bs ? dconst<NP>(0.0) : ld_dual(k.init_state[c + 1], a.dinit + (int64_t)(c + 1) * NP);
    }
    for (int t = 0; t < k.n_initial_store; ++t) ktp_store<NSLOT>(a, t, i, reg);
    const uint64_t path = k.path_offset + (uint64_t)i;
#pragma unroll 1
    for (int step = 0; step < k.n_steps; ++step) {
        const mcx_step sp = ldk_struct(&k.steps[step]);
        double z[NZ];
        if (INJECT) {
#pragma unroll
            for (int j = 0; j < NZ; ++j) z[j] = k.inject_z[((int64_t)step * NZ + j) * k.ld + i];
        } else {
#pragma unroll
            for (int q = 0; q < (NZ + 1) / 2; ++q) {
                double ua, z0, z1;
                draw_pair<true>(k.seed, path, (uint32_t)step, (uint32_t)q, ua, z0, z1, tab);
                z[2 * q] = z0;
                if (2 * q + 1 < NZ) z[2 * q + 1] = z1;
            }
        }
        const double* __restrict__ L = k.chol + (int64_t)sp.chol_idx * NZ * NZ;
        const double* __restrict__ dL = ca.dchol + (int64_t)sp.chol_idx * NZ * NZ * NP;
        const double dt = sp.dt;
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            DN zs = dconst<NP>(0.0);                                          // (L z)_s with the factor's tangent
#pragma unroll
            for (int c = 0; c <= s; ++c) zs = ktp_fma(ld_dual(ldk(L + s * NZ + c), dL + (int64_t)(s * NZ + c) * NP), z[c], zs);
            const DualKarg p{k.slots[s].p, a.dslot + (int64_t)s * MCX_SLOT_NPARAM * NP};
            const DualTable ax{k.aux + ((int64_t)step * NSLOT + s) * MCX_AUX, a.daux + ((int64_t)step * NSLOT + s) * MCX_AUX * NP};
            dual_step_analytical<false>(k.slots[s].kind == MCX_MODEL_BS, k.slots[s].kind, p, ax, dt, zs, reg[2 * s], reg[2 * s + 1]);
        }
        const int st = sp.store_idx;
        if (st >= 0) ktp_store<NSLOT>(a, st, i, reg);
    }
}

// The next variance of one Andersen QE step as a function of TWO numbers, vn = G(m, s2) (+ the draws u, z1), heston.py:185-236, in dual
// numbers with two directions (d/dm, d/ds2): the caller's parameter tangents follow by the chain rule, d vn = G_m d m + G_s2 d s2 —
// the ~30 operations of G carry 2 tangent components whatever the number of parameters.  Operation for operation the primal step
// (mcx_device.h step_slot): the seven reciprocals in three groups from one v_rcp_f64 each, the two roots of b2 as one, every
// denominator with the reference's eps, the NaN of a negative psi put in by hand.  A RESTATEMENT of the block in kt_heston
// (kt_tangent.hip:201-235): called from there as a shared function it changed that kernel's register allocation.
__device__ __forceinline__ Dual<2> ktp_qe_next_variance(double m, double s2, double u, double z1, bool fuzzy)
{
    const double eps = 1e-12;
    Dual<2> M, S2;
    M.v = m; M.d[0] = 1.0; M.d[1] = 0.0;
    S2.v = s2; S2.d[0] = 0.0; S2.d[1] = 1.0;
    const double omu = fmax(1.0 - u, eps);
    const Dual<2> d1 = M * M + eps, d5 = M + eps;
    const double d15 = d1.v * d5.v;
    const double ra = mcx_rcp(d15 * omu);
    const double r_omu = ra * d15, ra6 = ra * omu;
    const Dual<2> psi = ddiv_r(S2, d1, ra6 * d5.v);
    const Dual<2> d2 = psi + eps, d4 = psi + 1.0;
    const double rb = mcx_rcp(d2.v * d4.v);
    const Dual<2> invpsi = drcp_r(d2, rb * d4.v);
    const Dual<2> t = dclamp_min(invpsi * 2.0 - 1.0, 0.0);
    Dual<2> root = dsqrt(invpsi * 2.0 * t);
    if (invpsi.v < 0.0) root.v = __builtin_nan("");          // torch.sqrt(2 / psi) of a negative psi (mcx_device.h, QE step)
    const Dual<2> b2 = dclamp_min(invpsi * 2.0 - 1.0 + root, 0.0);
    const Dual<2> b = dsqrt(b2);
    const Dual<2> pp = dclamp(ddiv_r(psi - 1.0, d4, rb * d2.v), 0.0, 1.0 - 1e-6);
    const Dual<2> beta = ddiv_r(1.0 - pp, d5, ra6 * d1.v);
    const Dual<2> d3 = 1.0 + b2, d7 = beta + eps;
    const double rc = mcx_rcp(d3.v * d7.v);
    const Dual<2> aa = ddiv_r(M, d3, rc * d7.v);
    const Dual<2> bz = b + z1;
    const Dual<2> v1 = aa * bz * bz;
    const Dual<2> omp = dclamp_min(1.0 - pp, eps);
    const Dual<2> v_tail = ddiv_r(dlog(omp * r_omu), d7, rc * d3.v);
    const Dual<2> w_mass = ddegree(u - pp, fuzzy, 0.3);
    const Dual<2> v2 = w_mass * v_tail;
    const Dual<2> w = ddegree(psi - 1.5, fuzzy, 0.5);
    return (1.0 - w) * v1 + w * v2;
}

// kt_paths for a single Heston slot: state (log S, v), two normals per sub-step and, under QE, one uniform — K1's draws on K1's
// counters.  The tangent images run the step maps of step_slot (mcx_device.h) in dual numbers, operation for operation:
//   EULER (heston.py:109-121): the variance draw is row 1 of L z, L = chol([[1, rho], [rho, 1]]) — a dual row, value from k.chol and
//     tangent from dchol (the reference's tape differentiates through the factorisation); clamps pass the gradient on the closed side;
//   QE (heston.py:161-253): the aux row [E, K0, K1, K2, K3, K4, c1, c2] and its tangent row arrive through scalar loads, the map
//     vn = G(m, s2) runs in Dual<2> (ktp_qe_next_variance) and the NP tangents follow by the chain rule.
// The value image is not taken from the dual chain: step_slot itself advances the primal state, so image 0 is K1's arithmetic to the
// bit (under -ffp-contract=on the dual operators round product and sum separately where step_slot's expressions fuse them) and the
// frozen exercise policy of a dual pass sees the base run's values.  The price is a second evaluation of the step's value (~290
// instructions under QE) and, with Philox draws, 161 VGPRs / 3 waves per SIMD.  Within a step the clamp and indicator MASKS of the
// tangents are still taken from the dual chain's own unfused values, which start from the exact primal state but may differ from
// the stored value in the last bits (and dclamp_min keeps a NaN where the primal's `b2u < 0 ? 0 : b2u` does too, by another route):
// a path within rounding of a kink could carry the tangent of the other side.  That is the tie every float64 evaluation has at a
// kink; the tests keep their inputs 1e-9 away from every one of them.  Initial state and stores as kt_paths (ktp_store).
template <bool QE, bool INJECT>
__global__ __launch_bounds__(MCX_BLOCK) void kt_paths_heston(const KTPCholArgs ca)
{
    const KTPArgs& a = ca.p;
    const K1Args& k = a.k1;
    __shared__ double bm_lds[INJECT ? 2 : MCX_BM_LDS_DOUBLES];
    const double* tab = nullptr;
    if (!INJECT) { mcx_bm_load(bm_lds); tab = bm_lds; }
    const int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    if (i >= k.n) return;
    const int c0 = k.slots[0].state_off;
    DN reg[2];                                                                // (log S, v)
    reg[0] = ld_dual(k.init_state[c0], a.dinit + (int64_t)c0 * NP);
    reg[1] = ld_dual(k.init_state[c0 + 1], a.dinit + (int64_t)(c0 + 1) * NP);
    for (int t = 0; t < k.n_initial_store; ++t) ktp_store<1>(a, t, i, reg);
    const double* __restrict__ p = k.slots[0].p;                              // [spot, sigma_v, rate, rho, kappa, theta, v0]
    const double* __restrict__ dp = a.dslot;
    const int flags = k.flags | k.slots[0].flags;
    const uint64_t path = k.path_offset + (uint64_t)i;
#pragma unroll 1
    for (int step = 0; step < k.n_steps; ++step) {
        const mcx_step sp = ldk_struct(&k.steps[step]);
        double z0, z1, u = 0.0;
        if (INJECT) {
            z0 = k.inject_z[((int64_t)step * 2 + 0) * k.ld + i];
            z1 = k.inject_z[((int64_t)step * 2 + 1) * k.ld + i];
            if (QE) u = k.inject_u[(int64_t)step * k.ld + i];
        } else {
            double ua;
            draw_pair<true>(k.seed, path, (uint32_t)step, 0u, ua, z0, z1, tab);
            if (QE) { double t0, t1; draw_pair(k.seed, path, (uint32_t)step, 1u, u, t0, t1); }
        }
        const double dt = sp.dt, sq = sp.sqrt_dt;
        const double* __restrict__ ax = k.aux + (int64_t)step * MCX_AUX;
        // row 1 of the ONE factor of an EULER / QE run (sim_apply: L00 = 1 exactly, QE's factor is the identity)
        const double l10 = ldk(k.chol + 2), l11 = ldk(k.chol + 3);
        double s0 = reg[0].v, s1 = reg[1].v;                                  // image 0: the primal step itself
        step_slot<MCX_MODEL_HESTON, QE ? MCX_SCHEME_QE : MCX_SCHEME_EULER>(k.slots[0], k.scheme, flags, dt, sq, AuxPtr{ax}, s0, s1, z0,
                                                                           fma(l11, z1, l10 * z0), u);
        const DN rate = ld_dual(p[2], dp + 2 * NP), theta = ld_dual(p[5], dp + 5 * NP);
        const DN v = reg[1];
        DN vn;
        if constexpr (!QE) {
            const DN sigma = ld_dual(p[1], dp + 1 * NP), kappa = ld_dual(p[4], dp + 4 * NP);
            const DN zc1 = ktp_fma(ld_dual(l11, ca.dchol + 3 * NP), z1, ld_dual(l10, ca.dchol + 2 * NP) * z0);
            const DN sv = dsqrt(dclamp_min(v, 0.0));
            reg[0] = reg[0] + (rate - v * 0.5) * dt + sv * (sq * z0);
            vn = dclamp_min(v + kappa * (theta - v) * dt + sigma * sv * sq * zc1, 0.0);
        } else {
            const double* __restrict__ dax = a.daux + (int64_t)step * MCX_AUX * NP;
            auto aux = [&](int e) __attribute__((always_inline)) { return ld_dual(ldk(ax + e), dax + e * NP); };
            const double eps = 1e-12;
            const DN m = theta + (v - theta) * aux(0);
            const DN s2 = v * aux(6) + aux(7);
            const Dual<2> vn2 = ktp_qe_next_variance(m.v, s2.v, u, z1, (flags & MCX_FLAG_SMOOTHING) != 0);
            vn.v = vn2.v;
#pragma unroll
            for (int q = 0; q < NP; ++q) vn.d[q] = fma(vn2.d[0], m.d[q], vn2.d[1] * s2.d[q]);
            const DN var_int = dclamp_min(aux(4) * v + aux(5) * vn, 0.0);     // (K4 v_next counts: the primal reads aux[5])
            const DN vol = dsqrt(dclamp_min(var_int, eps));
            reg[0] = reg[0] + rate * dt + aux(1) + aux(2) * v + aux(3) * vn + vol * z0;
        }
        reg[1] = vn;
        reg[0].v = s0;
        reg[1].v = s1;
        const int st = sp.store_idx;
        if (st >= 0) ktp_store<1>(a, st, i, reg);
    }
}

// ---- dual atoms ---------------------------------------------------------------------------------------------------------
struct KTBook {
    const DevTerm* __restrict__ terms;
    const DevEvent* __restrict__ events;
    const DevAtom* __restrict__ atoms;
    const DevEventIds* __restrict__ ev_ids;   // DevEvent and DevTerm carry COPIES of their atoms: the ids behind them find the
    const int32_t* __restrict__ term_atom;    // derivative rows ([n_events], [n_terms]; the book's, mcx_book_tangent_ids)
    const double* __restrict__ datoms;   // [n_atoms][5][NP]: d(a, d, b, c0, c1) / d theta
    const double* __restrict__ paths;
    const double* __restrict__ dpaths;
    int64_t n, ld, pstride;
    int32_t n_state, n_basis;
};

__device__ __forceinline__ DN kt_atom(const KTBook& b, const DevAtom& a, int atom_id, int64_t i)
{
    const double* __restrict__ da = b.datoms + (int64_t)atom_id * 5 * NP;
    DN x = dconst<NP>(0.0);
    if (a.col >= 0) x = dload<NP>(b.paths, b.dpaths, b.pstride, ((int64_t)a.t_idx * b.n_state + a.col) * b.ld + i);
    DN v = ld_dual(a.a, da) + ld_dual(a.d, da + NP) * x;
    if (a.b != 0.0) v = v + ld_dual(a.b, da + 2 * NP) * dexp(ld_dual(a.c0, da + 3 * NP) + ld_dual(a.c1, da + 4 * NP) * x);
    return v;
}

// sum of an event's weighted dual terms; the terms over a denominator of their own (mcx_term.den, the unequal-tenor swap quirk) go
// to `own`.  Only CASHFLOW events have such terms: the host refuses them under OPTION and EXERCISE events (kt_tangent_form)
__device__ __forceinline__ DN kt_term_sum(const KTBook& b, const DevEvent& e, int64_t i, DN& own)
{
    DN val = dconst<NP>(0.0);
    own = dconst<NP>(0.0);
    for (int j = e.term_begin; j < e.term_end; ++j) {
        const DevTerm tm = ldk_struct(&b.terms[j]);
        const DN v = kt_atom(b, tm.atom, ldk(b.term_atom + j), i) * tm.w;
        if (tm.den < 0) val = val + v;
        else own = own + v / kt_atom(b, ldk_struct(&b.atoms[tm.den]), tm.den, i);
    }
    return val;
}

// ---- payoff forms in dual numbers: MCX_EV_OPTION in the aggregation modes 1-5 ---------------------------------------------------
// Each form restates its primal (k2_book.hip dev_cash_event, mcx_device.h dev_barrier_event) operation for operation, so the value
// image is the primal's, and follows the reference's tape: the indicators are fuzzy (clamp: the gradient passes on the closed band,
// dclamp), torch.max / torch.min over the monitored spots hand the gradient to the FIRST extremal spot in monitoring order, the
// bridge uniforms carry no tangent.  The one host-computed number of an event — the closed-form geometric price aux[1] of mode 2, the
// bridge constant c = -2 / (sigma^2 maturity / n_obs) of mode 5 — takes its tangent from row q of `dpayoff`
// (mcx_book_set_payoff_tangents).  Compiled only into the EXOTIC instantiations of the kernels: the others keep their code.
struct KTPayoff {
    const double* __restrict__ coeffs;     // the book's coefficient array: (c, draw id) of a bridge event at its coeff_off
    const double* __restrict__ dpayoff;    // [n_events][NP]
    const DevBridge* __restrict__ bridge;  // RNG state of the bridge draws (mcx_book_set_bridge_rng): the primal kernels' numbers
};

__device__ __forceinline__ DN kt_wfma(double w, const DN& a, const DN& acc)       // acc + w a, every image one multiply-add
{
    DN r;
    r.v = fma(w, a.v, acc.v);
#pragma unroll
    for (int q = 0; q < NP; ++q) r.d[q] = fma(w, a.d[q], acc.d[q]);
    return r;
}
__device__ __forceinline__ DN kt_divc(const DN& a, double c)                      // a / c with the primal's true division in the value
{
    DN r;
    r.v = a.v / c;
    const double ic = 1.0 / c;
#pragma unroll
    for (int q = 0; q < NP; ++q) r.d[q] = a.d[q] * ic;
    return r;
}
// fuzzy indicator with eps = 0.05 (maths.py:8) as the primal writes it: clamp((x + 0.05) / 0.1, 0, 1)
__device__ __forceinline__ DN kt_fuzzy(const DN& x) { return dclamp(kt_divc(x + 0.05, 0.1), 0.0, 1.0); }
// barrier indicator of one level (dev_barrier_ind): 1 up-and-out, 2 down-and-out, 3 up-and-in, 4 down-and-in
__device__ __forceinline__ DN kt_barrier_ind(int type, double level, const DN& mx, const DN& mn)
{
    const DN ind = (type & 1) ? kt_fuzzy(level - mx) : kt_fuzzy(mn - level);
    return type <= 2 ? ind : 1.0 - ind;
}

__device__ __forceinline__ DN kt_barrier_event(const KTBook& b, const KTPayoff& px, const DevEvent& e, const DevEventIds& id, int q, int64_t i)
{
    const int types = (int)e.aux[3];
    const int t1 = types & 7, t2 = types >> 3;
    const bool with_bridge = e.aux[0] == 5.0;
    DN mx = dconst<NP>(-1.0e300), mn = dconst<NP>(1.0e300), keep1 = dconst<NP>(1.0), keep2 = dconst<NP>(1.0);
    DN prev1 = dconst<NP>(0.0), prev2 = dconst<NP>(0.0), c = dconst<NP>(0.0);
    int draw_id = 0;
    DevBridge br = {0, 0, nullptr, 0};
    const double* __restrict__ inj = nullptr;
    if (with_bridge) {
        c = ld_dual(ldk(px.coeffs + e.coeff_off), px.dpayoff + (int64_t)q * NP);
        draw_id = (int)ldk(px.coeffs + e.coeff_off + 1);
        br = ldk_struct(px.bridge);
        if (br.inject) inj = br.inject[draw_id];
    }
    for (int j = e.term_begin; j < e.term_end; ++j) {
        const DN s = kt_atom(b, ldk_struct(&b.terms[j]).atom, ldk(b.term_atom + j), i);
        if (s.v > mx.v) mx = s;                              // strict: the first extremal spot keeps the gradient
        if (s.v < mn.v) mn = s;
        if (with_bridge) {
            const DN cur1 = dlog(kt_divc(s, e.aux[1])), cur2 = t2 ? dlog(kt_divc(s, e.aux[2])) : dconst<NP>(0.0);
            if (j > e.term_begin) {
                const int k = j - e.term_begin - 1;          // interval index
                for (int bi = 0; bi < (t2 ? 2 : 1); ++bi) {
                    const DN p = dexp(c * (bi ? prev2 * cur2 : prev1 * cur1));
                    double u;
                    if (inj) u = inj[(int64_t)(2 * k + bi) * br.ld + i];
                    else {
                        uint32_t w0, w1, w2, w3;
                        const uint64_t path = br.path_offset + (uint64_t)i;
                        philox4x32_10((uint32_t)path, (uint32_t)(path >> 32), (uint32_t)k, 0x80000000u | (uint32_t)(2 * draw_id + bi),
                                      (uint32_t)br.seed, (uint32_t)(br.seed >> 32), w0, w1, w2, w3);
                        u = u53(w0, w1);
                    }
                    const DN miss = 1.0 - kt_fuzzy(p - u);   // 1 - compute_degree_of_truth(p - u, True)
                    if (bi) keep2 = keep2 * miss; else keep1 = keep1 * miss;
                }
            }
            prev1 = cur1; prev2 = cur2;
        }
    }
    DN pay = dmax0((kt_atom(b, e.x, id.x, i) - e.strike) * e.sign) * kt_barrier_ind(t1, e.aux[1], mx, mn);
    if (with_bridge) pay = pay * ((t1 <= 2) ? keep1 : 1.0 - keep1);       // out: never hit; in: hit at least once
    if (t2) {
        pay = pay * kt_barrier_ind(t2, e.aux[2], mx, mn);
        if (with_bridge) pay = pay * ((t2 <= 2) ? keep2 : 1.0 - keep2);
    }
    return pay / kt_atom(b, e.num, id.num, i);
}

// modes 1 (geometric aggregate), 2 (arithmetic with the geometric control variate), 3 (binary); 4 / 5 above
__device__ __forceinline__ DN kt_payoff_event(const KTBook& b, const KTPayoff& px, const DevEvent& e, const DevEventIds& id, int q, int64_t i)
{
    if (e.aux[0] == 4.0 || e.aux[0] == 5.0) return kt_barrier_event(b, px, e, id, q, i);
    const DN num = kt_atom(b, e.num, id.num, i);
    const bool binary = e.aux[0] == 3.0;
    DN val = dconst<NP>(0.0), glog = dconst<NP>(0.0);
    for (int j = e.term_begin; j < e.term_end; ++j) {
        const DevTerm tm = ldk_struct(&b.terms[j]);
        const DN av = kt_atom(b, tm.atom, ldk(b.term_atom + j), i);
        if (binary) { val = kt_wfma(tm.w, av, val); continue; }
        val = val + av * tm.w;
        glog = kt_wfma(tm.w, dlog(av + 1e-10), glog);                     // basket_option.py:62-65
    }
    if (binary) {                                                         // binary_option.py:38-43
        const DN dot = dclamp(kt_divc(val - e.strike + e.aux[2], 2.0 * e.aux[2]), 0.0, 1.0);
        return ((e.sign > 0.0 ? dot : 1.0 - dot) * e.aux[1]) / num;
    }
    const DN geo = dmax0((dexp(glog) - e.strike) * e.sign);
    if (e.aux[0] == 1.0) return geo / num;
    const DN imm = dmax0((val - e.strike) * e.sign);                      // basket_option.py:72-78
    return (imm - geo + ld_dual(e.aux[1], px.dpayoff + (int64_t)q * NP)) / num;
}

// normalised dual cashflow of one stateless cash event q (CASHFLOW or OPTION; the payoff modes only where EXOTIC)
template <bool EXOTIC = false>
__device__ __forceinline__ DN kt_cash_event(const KTBook& b, const DevEvent& e, const DevEventIds& id, int64_t i, const KTPayoff* px = nullptr,
                                            int q = 0)
{
    if (EXOTIC && e.kind == MCX_EV_OPTION && e.aux[0] != 0.0) return kt_payoff_event(b, *px, e, id, q, i);
    const DN num = kt_atom(b, e.num, id.num, i);
    DN own;
    const DN val = kt_term_sum(b, e, i, own);
    if (e.kind == MCX_EV_CASHFLOW) return val / num + own;
    const DN pay = dmax0((val - e.strike) * e.sign);
    return pay / num;
}

// ---- exercise events in dual numbers -------------------------------------------------------------------------------------------
// The reference's tape puts NO gradient through the boolean `should_exercise` (bermudan_option.py:122-128; flexicall.py:118-133):
// the decision is taken from the primal values — immediate value against the regression continuation value of the path's state —
// and the tangent flows through the branch that was taken only (the immediate value, where the path exercises).
// State-independent pieces of one MCX_EV_EXERCISE event for path i: the dual immediate value already divided by the numeraire and
// the primal explanatory variable of the continuation polynomial.
struct KTExercise { DN pay; double imm, x; };
__device__ __forceinline__ KTExercise kt_exercise_value(const KTBook& b, const DevEvent& e, const DevEventIds& id, int64_t i)
{
    KTExercise r;
    const DN num = kt_atom(b, e.num, id.num, i);
    DN own;
    const DN val = kt_term_sum(b, e, i, own);
    const DN imm = dmax0((val - e.strike) * e.sign);
    r.pay = imm / num;
    r.imm = imm.v;
    r.x = e.coeff_off >= 0 ? kt_atom(b, e.x, id.x, i).v : 0.0;
    return r;
}
__device__ __forceinline__ double kt_poly(const double* __restrict__ c, int K, double x)
{
    double v = 0.0, xp = 1.0;
    for (int k = 0; k < K; ++k) { v = fma(c[k], xp, v); xp *= x; }
    return v;
}
// decision of a path in state s (the PRIMAL coefficients of the base run: the same decisions as its primal pass); s is decremented
__device__ __forceinline__ bool kt_exercises(const DevEvent& e, const double* __restrict__ coeffs, int K, const KTExercise& ev, int& s)
{
    double cont = 0.0, cont_ex = 0.0;
    if (e.coeff_off >= 0) {
        cont = kt_poly(coeffs + e.coeff_off + s * K, K, ev.x);
        if (e.aux[0] == 1.0 && s > 0) cont_ex = kt_poly(coeffs + e.coeff_off + (s - 1) * K, K, ev.x);      // flexicall.py:118-133
    }
    const bool ex = (ev.imm + cont_ex > cont) && (s > 0);
    if (ex) s -= 1;
    return ex;
}

// ---- LSM moments with tangents ------------------------------------------------------------------------------------------
// moments of a regression date over S hypothetical states, [1+NP][(2K-1) + S K] per lane in registers: the powers z^0 .. z^(2K-2)
// of the normalised explanatory variable (Gram matrix), then z^k (num w[s]) for k < K (right-hand side of state s)
template <int K, int S>
__device__ __forceinline__ void kt_moments_add(double (&acc)[1 + NP][(2 * K - 1) + S * K], const DN& z, const DN& num, const DN (&w)[S])
{
    DN zp = dconst<NP>(1.0);
#pragma unroll
    for (int k = 0; k < 2 * K - 1; ++k) {
        acc[0][k] += zp.v;
#pragma unroll
        for (int q = 0; q < NP; ++q) acc[1 + q][k] += zp.d[q];
        if (k < K) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const DN zy = zp * (num * w[s]);
                acc[0][(2 * K - 1) + s * K + k] += zy.v;
#pragma unroll
                for (int q = 0; q < NP; ++q) acc[1 + q][(2 * K - 1) + s * K + k] += zy.d[q];
            }
        }
        zp = zp * z;
    }
}
// the block's sums of every moment to `partials` [1+NP][NM] (the caller's tile)
template <int NM>
__device__ __forceinline__ void kt_moments_store(const double (&acc)[1 + NP][NM], double* __restrict__ partials)
{
    __shared__ double lds[4];
#pragma unroll
    for (int q = 0; q <= NP; ++q)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const double r = block_sum(acc[q][m], lds);
            if (threadIdx.x == 0) partials[q * NM + m] = r;
        }
}

// ---- LSM step of an exercise product with tangents: the cashflow cache is rolled one window back along the frozen policy ----------
// (controller.py:316-383; K3's k3_roll in dual numbers).  W [S][ld_w] and dW [NP][S][ld_w] hold, per hypothetical state, the
// discounted cashflows after the previous regression date and their tangents; moments [1+NP][(2K-1) + S K].
struct KTSArgs {
    KTBook b;
    const double* __restrict__ coeffs;         // primal coefficients of the base run (decisions)
    double* __restrict__ W;
    double* __restrict__ dW;
    DevAtom num, x;
    double shift, scale;
    double* __restrict__ partials;             // [gridDim.x][1+NP][NM]
    int64_t ld_w, w_stride;                    // w_stride = S * ld_w (between tangents)
    int32_t roll_begin, roll_end, num_id, x_id;
};

template <int K, int S>
__global__ __launch_bounds__(MCX_BLOCK) void kt_lsm_step(const KTSArgs a)
{
    constexpr int NM = (2 * K - 1) + S * K;
    double acc[1 + NP][NM];
#pragma unroll
    for (int q = 0; q <= NP; ++q)
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[q][m] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x; i < a.b.n; i += (int64_t)gridDim.x * MCX_BLOCK) {
        DN w[S];
#pragma unroll
        for (int s = 0; s < S; ++s) w[s] = dload<NP>(a.W, a.dW, a.w_stride, (int64_t)s * a.ld_w + i);
        if (a.roll_end > a.roll_begin) {
            int st[S];
            DN sv[S];
#pragma unroll
            for (int s0 = 0; s0 < S; ++s0) { st[s0] = s0; sv[s0] = dconst<NP>(0.0); }
            for (int q = a.roll_begin; q < a.roll_end; ++q) {                   // controller.py:333-341
                const DevEvent e = ldk_struct(&a.b.events[q]);
                const DevEventIds id = ldk_struct(&a.b.ev_ids[q]);
                if (e.kind == MCX_EV_EXERCISE) {
                    const KTExercise ev = kt_exercise_value(a.b, e, id, i);      // once per path and date, not per state
#pragma unroll
                    for (int s0 = 0; s0 < S; ++s0)
                        if (kt_exercises(e, a.coeffs, K, ev, st[s0])) sv[s0] = sv[s0] + ev.pay;
                } else {
                    const DN v = kt_cash_event(a.b, e, id, i);
#pragma unroll
                    for (int s0 = 0; s0 < S; ++s0) sv[s0] = sv[s0] + v;
                }
            }
            DN wn[S];
#pragma unroll
            for (int s0 = 0; s0 < S; ++s0) {
                DN tail = w[0];
#pragma unroll
                for (int q = 1; q < S; ++q) if (st[s0] == q) tail = w[q];        // lookup_state_values (product.py:150-155)
                wn[s0] = sv[s0] + tail;
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
                w[s] = wn[s];
                dstore(a.W, a.dW, a.w_stride, (int64_t)s * a.ld_w + i, wn[s]);
            }
        }
        const DN num = kt_atom(a.b, a.num, a.num_id, i);                                   // :368
        const DN z = (kt_atom(a.b, a.x, a.x_id, i) - a.shift) * a.scale;
        kt_moments_add<K, S>(acc, z, num, w);
    }
    kt_moments_store<NM>(acc, a.partials + (int64_t)blockIdx.x * ((1 + NP) * NM));
}

// ---- LSM moments of stateless products ---------------------------------------------------------------------------------------
// one (product, regression date): the flattened numeraire / explanatory atoms, their ids and the product's cash events it sums
struct KTLJob {
    DevAtom num, x;
    double shift, scale;
    int32_t ev_first, ev_end, num_id, x_id;
};
struct KTLBatchArgs {
    KTBook b;
    const KTLJob* __restrict__ jobs;           // [gridDim.y] the jobs of this launch
    double* __restrict__ partials;             // [gridDim.y][gridDim.x][(1+NP)][NM]
};
// the arguments of a kernel's EXOTIC instantiation: the plain ones, then the payoff state.  The plain instantiation keeps the plain
// record, and with it the layout of its kernel arguments
template <class Args> struct KTWithPayoff { Args a; KTPayoff px; };
template <class Args, bool EXOTIC> using KTArgsOf = std::conditional_t<EXOTIC, KTWithPayoff<Args>, Args>;
template <class Args> __device__ __forceinline__ const Args& kt_plain(const Args& a) { return a; }
template <class Args> __device__ __forceinline__ const Args& kt_plain(const KTWithPayoff<Args>& x) { return x.a; }
template <class Args> __device__ __forceinline__ const KTPayoff* kt_payoff_of(const Args&) { return nullptr; }
template <class Args> __device__ __forceinline__ const KTPayoff* kt_payoff_of(const KTWithPayoff<Args>& x) { return &x.px; }

// grid (tiles, jobs): block (t, j) takes the paths t, t + tiles, ... of job j in blocks of MCX_BLOCK, so the order of every sum of
// a job depends on the path count alone, not on the jobs around it.  The job is wave-uniform: its record arrives through scalar
// loads, as the events do.
template <int K, bool EXOTIC>
__global__ __launch_bounds__(MCX_BLOCK) void kt_lsm_batch(const KTArgsOf<KTLBatchArgs, EXOTIC> ax)
{
    const KTLBatchArgs& a = kt_plain(ax);
    constexpr int NM = (2 * K - 1) + K;
    const KTLJob j = ldk_struct(&a.jobs[blockIdx.y]);
    double acc[1 + NP][NM];
#pragma unroll
    for (int q = 0; q <= NP; ++q)
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[q][m] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x; i < a.b.n; i += (int64_t)gridDim.x * MCX_BLOCK) {
        DN total[1] = {dconst<NP>(0.0)};
        for (int q = j.ev_first; q < j.ev_end; ++q)                                       // controller.py:333-352 without the cache
            total[0] = total[0] + kt_cash_event<EXOTIC>(a.b, ldk_struct(&a.b.events[q]), ldk_struct(&a.b.ev_ids[q]), i, kt_payoff_of(ax), q);
        const DN num = kt_atom(a.b, j.num, j.num_id, i);                                   // :368
        const DN z = (kt_atom(a.b, j.x, j.x_id, i) - j.shift) * j.scale;
        kt_moments_add<K, 1>(acc, z, num, total);
    }
    kt_moments_store<NM>(acc, a.partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ((1 + NP) * NM));
}

// ---- book evaluation with tangents ----------------------------------------------------------------------------------------
struct KTEArgs {
    KTBook b;
    const DevProduct* __restrict__ products;
    const double* __restrict__ coeffs;         // [n_coeffs] regression coefficients of the tangent pass
    const double* __restrict__ dcoeffs;        // [n_coeffs][NP]
    double* __restrict__ cfs;                  // [1+NP][n_ns][ld]   (zero-initialised)
    double* __restrict__ expo;                 // [1+NP][n_ns][n_rows][ld] (zero-initialised)
    const int32_t* __restrict__ ev_param;      // [n_events][2] tangent slot (0..NP-1 or -1) of an EXPO_BS event's sigma / rate; nullable
    int32_t n_products, n_ns, n_rows, pad;
};

template <bool EXOTIC>
__global__ __launch_bounds__(MCX_BLOCK) void kt_eval(const KTArgsOf<KTEArgs, EXOTIC> ax)
{
    const KTEArgs& a = kt_plain(ax);
    const int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    if (i >= a.b.n) return;
    const int K = a.b.n_basis;
    const int64_t cf_stride = (int64_t)a.n_ns * a.b.ld, ex_stride = (int64_t)a.n_ns * a.n_rows * a.b.ld;
    for (int p = 0; p < a.n_products; ++p) {
        const DevProduct pr = ldk_struct(&a.products[p]);
        DN acc = dconst<NP>(0.0);
        int state = pr.init_state;                                                        // rights left (exercise products)
        for (int q = pr.ev_begin; q < pr.ev_end; ++q) {
            const DevEvent e = ldk_struct(&a.b.events[q]);
            const DevEventIds id = ldk_struct(&a.b.ev_ids[q]);
            if (e.kind <= MCX_EV_OPTION) {
                acc = acc + kt_cash_event<EXOTIC>(a.b, e, id, i, kt_payoff_of(ax), q);
            } else if (e.kind == MCX_EV_EXERCISE) {
                // decision from the primal values, tangent through the taken branch only (bermudan_option.py:93-131)
                const KTExercise ev = kt_exercise_value(a.b, e, id, i);
                if (kt_exercises(e, a.coeffs, K, ev, state)) acc = acc + ev.pay;
            } else {                                                                      // exposures (controller.py:430-447)
                DN v = dconst<NP>(0.0);
                if (e.kind == MCX_EV_EXPO_BS) {
                    // analytic Black-Scholes exposure (european_option.py:123-145) in dual numbers: sigma and rate are model
                    // parameters (their tangent slots come from the host), the spot is the path state
                    if (e.aux[2] > 0.0) {
                        DN sig = dconst<NP>(e.aux[0]), rate = dconst<NP>(e.aux[1]);
                        const int s_sig = a.ev_param ? ldk(a.ev_param + 2 * q) : -1, s_rate = a.ev_param ? ldk(a.ev_param + 2 * q + 1) : -1;
#pragma unroll
                        for (int r = 0; r < NP; ++r) { sig.d[r] = (r == s_sig) ? 1.0 : 0.0; rate.d[r] = (r == s_rate) ? 1.0 : 0.0; }
                        const double tau = e.aux[2], sq = sqrt(tau);
                        const DN spot = kt_atom(a.b, e.x, id.x, i);
                        const DN d1 = (dlog(spot * (1.0 / e.strike)) + (rate + sig * sig * 0.5) * tau) / (sig * sq);
                        const DN d2 = d1 - sig * sq;
                        const DN df = dexp(rate * (-tau));
                        auto ncdf = [](const DN& x) {                      // Phi(x), d Phi = phi(x) dx
                            DN r;
                            r.v = 0.5 * (1.0 + erf(x.v * 0.70710678118654752440));
                            const double pdf = 0.39894228040143267794 * exp(-0.5 * x.v * x.v);
#pragma unroll
                            for (int q2 = 0; q2 < NP; ++q2) r.d[q2] = pdf * x.d[q2];
                            return r;
                        };
                        const DN price = e.sign > 0.0 ? spot * ncdf(d1) - df * ncdf(d2) * e.strike
                                                      : df * ncdf(d2 * -1.0) * e.strike - spot * ncdf(d1 * -1.0);
                        v = price / kt_atom(a.b, e.num, id.num, i);
                    }
                } else if (e.coeff_off >= 0) {
                    const DN x = kt_atom(a.b, e.x, id.x, i);
                    DN xp = dconst<NP>(1.0);
                    // the coefficient row of the path's exercise state (product.py:150-184); stateless products: row 0
                    const int row0 = e.coeff_off + (pr.n_states > 1 ? state * K : 0);
                    for (int k = 0; k < K; ++k) {
                        const DN ck = dload<NP>(a.coeffs + (row0 + k), a.dcoeffs + (int64_t)(row0 + k) * NP, 1, 0);
                        v = v + ck * xp;
                        xp = xp * x;
                    }
                    v = v / kt_atom(a.b, e.num, id.num, i);
                }
                dadd(a.expo, a.expo + ex_stride, ex_stride, ((int64_t)pr.netting_set * a.n_rows + e.row) * a.b.ld + i, v);
            }
        }
        dadd(a.cfs, a.cfs + cf_stride, cf_stride, (int64_t)pr.netting_set * a.b.ld + i, acc);
    }
}

// ---- CVA with tangents ------------------------------------------------------------------------------------------------------
// unsecured exposure of one netting set at metric date m with tangents (netting_set.py:48-72, 156-184; mcx_unsecured_desc):
//   not collateralised: thr(E[row]);   collateralised: E[row] - thr(E[delayed]) (delayed < 0: no collateral yet)
__device__ __forceinline__ DN kt_thr(const DN& e, double h)
{
    if (h == 0.0) return e;
    DN r = e;
    if (e.v > h) r.v = e.v - h;
    else if (e.v < -h) r.v = e.v + h;
    else r = dconst<NP>(0.0);
    return r;
}
__device__ __forceinline__ DN kt_unsecured(const double* __restrict__ expo, int64_t ex_stride, const int32_t* __restrict__ rows,
                                           const int32_t* __restrict__ delayed, int collateralized, double h, int64_t ld, int m, int64_t i)
{
    const DN e = dload<NP>(expo, expo + ex_stride, ex_stride, (int64_t)ldk(rows + m) * ld + i);
    if (!collateralized) return kt_thr(e, h);
    if (!delayed) return e;
    const int dm = ldk(delayed + m);
    if (dm < 0) return e;
    return e - kt_thr(dload<NP>(expo, expo + ex_stride, ex_stride, (int64_t)dm * ld + i), h);
}

struct KTCArgs {
    KTBook b;
    const double* __restrict__ expo;           // [1+NP][n_rows][ld] of ONE netting set (stride ex_stride between tangents)
    const int32_t* __restrict__ rows;          // [n_dates] exposure row of every metric date
    const int32_t* __restrict__ delayed;       // [n_dates] delayed (t - MPoR) row or -1; nullptr when not collateralised
    const int32_t* __restrict__ surv;          // [n_dates-1] atom ids
    const int32_t* __restrict__ cond;
    double* __restrict__ out;                  // [1+NP][ld]
    int64_t ex_stride;
    double threshold, lgd;
    int32_t n_dates, collateralized;
};

__global__ __launch_bounds__(MCX_BLOCK) void kt_cva(const KTCArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    if (i >= a.b.n) return;
    DN cva = dconst<NP>(0.0);
    for (int m = 0; m < a.n_dates - 1; ++m) {                                             // cva_metric.py:78-96
        const DN pos = kt_unsecured(a.expo, a.ex_stride, a.rows, a.delayed, a.collateralized, a.threshold, a.b.ld, m, i);
        if (!(pos.v > 0.0)) continue;                    // relu: gradient passes where the unsecured exposure is positive
        const int sa = ldk(a.surv + m), ca = ldk(a.cond + m);
        const DN sp = kt_atom(a.b, ldk_struct(&a.b.atoms[sa]), sa, i);
        const DN cs = kt_atom(a.b, ldk_struct(&a.b.atoms[ca]), ca, i);
        cva = cva + pos * sp * (1.0 - cs);
    }
    dstore(a.out, a.out + a.b.ld, a.b.ld, i, cva * a.lgd);
}

// ---- bilateral xVA with tangents: the dual of k4_xva (k4_xva.hip) ---------------------------------------------------------------
// Per path, c the counterparty, o the own name, x_m the dual unsecured exposure and the sums over m = 0 .. n_dates-2:
//   cva = lgd_c sum pos(x_m) S_c q_c      dva = lgd_o sum neg(x_m) S_o q_o      cva_ftd = lgd_c sum pos(x_m) (S_c q_c) S_o
//   dva_ftd = lgd_o sum neg(x_m) (S_o q_o) S_c      bcva = cva_ftd - dva_ftd
// pos(x) = x where x.v > 0, neg(x) = -x where x.v < 0, both zero (value and tangents) at x.v == 0: torch.relu, as kt_cva.
// A lane owns a path (grid stride), walks the dates once and keeps the four dual accumulators in registers; the 5 (1+NP) plain sums
// over the block's paths follow in the same launch: wave shuffles, then the wave totals of every entry added in wave order by one
// thread per entry; one partial per block, no float atomics.  The products are written as k4_xva writes them (S q first, then times
// the other name's S, lgd at the end), so that swapping the names and negating every exposure image runs the same arithmetic on
// the other accumulator; bcva is the difference of the two scaled legs in a statement of its own (no contraction).
// The reduction uses wave_sum and a [4 waves][25] table in LDS (800 B) behind ONE barrier, not block_sum: that helper takes two
// barriers per entry, 50 for the 25 sums.
#define KTX_R 5                                  // records: cva, dva, cva_ftd, dva_ftd, bcva
#define KTX_N (KTX_R * (1 + NP))                 // sums per block: [record][image]
// blocks of one launch.  The kernel holds 2 waves per SIMD (169 VGPRs, profiles/xva_tangent_resource_usage.txt: the 25 sums, four
// dual accumulators, the dual weights and the dual exposure are live in the date loop; forcing 3 or 4 waves spills to scratch), i.e.
// 2 blocks of 4 waves per CU: 2 x 256 CUs of the MI355X fill every wave slot the kernel can hold in ONE round, and more paths than
// 512 x 256 take the grid stride.  A constant, not a multiple of the device's CU count: the partials [grid][25] and their sum fit
// the workspace on every device, and the sums of a book do not depend on the device's size
constexpr int KT_XVA_GRID_CAP = 512;
// the partials of a full grid fit the handle's workspace and its pinned buffer: mcx_tangent_xva's workspace refusal cannot be reached
static_assert(sizeof(double) * KT_XVA_GRID_CAP * KTX_N <= MCX_WS_BYTES && sizeof(double) * KT_XVA_GRID_CAP * KTX_N <= MCX_PINNED_BYTES,
              "kt_xva: the block partials of a full grid exceed the handle's workspace or pinned buffer");

struct KTXSide {                                 // one name: atom ids per date (device, [n_dates-1]); surv == nullptr: never defaults
    const int32_t* __restrict__ surv;
    const int32_t* __restrict__ cond;
    double lgd;
};

struct KTXArgs {
    KTBook b;
    const double* __restrict__ expo;           // [1+NP][n_rows][ld] of ONE netting set (stride ex_stride between tangents)
    const int32_t* __restrict__ rows;
    const int32_t* __restrict__ delayed;
    KTXSide c, o;
    double* __restrict__ partials;             // [gridDim.x][KTX_R][1+NP]
    int64_t ex_stride;
    double threshold;
    int32_t n_dates, collateralized;
};

// S(0, t_m) and q = 1 - S(t_m, t_m+1) of one name; a name without atoms: the dual constants 1 and 0
__device__ __forceinline__ void ktx_side(const KTBook& b, const KTXSide& s, int m, int64_t i, DN& S, DN& q)
{
    S = dconst<NP>(1.0); q = dconst<NP>(0.0);
    if (s.surv) {                                                   // wave-uniform
        const int sa = ldk(s.surv + m), ca = ldk(s.cond + m);
        S = kt_atom(b, ldk_struct(&b.atoms[sa]), sa, i);
        q = 1.0 - kt_atom(b, ldk_struct(&b.atoms[ca]), ca, i);
    }
}

__global__ __launch_bounds__(MCX_BLOCK) void kt_xva(const KTXArgs a)
{
    __shared__ double wsum[MCX_BLOCK / MCX_WAVE][KTX_N];
    double acc[KTX_N];
#pragma unroll
    for (int k = 0; k < KTX_N; ++k) acc[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x; i < a.b.n; i += (int64_t)gridDim.x * MCX_BLOCK) {
        DN cva = dconst<NP>(0.0), dva = dconst<NP>(0.0), cftd = dconst<NP>(0.0), dftd = dconst<NP>(0.0);
        for (int m = 0; m < a.n_dates - 1; ++m) {
            const DN x = kt_unsecured(a.expo, a.ex_stride, a.rows, a.delayed, a.collateralized, a.threshold, a.b.ld, m, i);
            DN ep = dconst<NP>(0.0), en = dconst<NP>(0.0);          // relu: the gradient passes where the leg is strictly positive
            if (x.v > 0.0) ep = x;
            else if (x.v < 0.0) en = 0.0 - x;
            // one name's two atoms at a time: q is dead once the weight S q is formed (the live set decides the occupancy)
            DN Sc, So, q;
            ktx_side(a.b, a.c, m, i, Sc, q);
            const DN wc = Sc * q;
            ktx_side(a.b, a.o, m, i, So, q);
            const DN wo = So * q;
            cva = cva + ep * wc;
            dva = dva + en * wo;
            cftd = cftd + ep * (wc * So);
            dftd = dftd + en * (wo * Sc);
        }
        DN v[KTX_R];
        v[0] = cva * a.c.lgd;
        v[1] = dva * a.o.lgd;
        v[2] = cftd * a.c.lgd;
        v[3] = dftd * a.o.lgd;
        v[4] = v[2] - v[3];
#pragma unroll
        for (int r = 0; r < KTX_R; ++r) {
            acc[r * (1 + NP)] += v[r].v;
#pragma unroll
            for (int q = 0; q < NP; ++q) acc[r * (1 + NP) + 1 + q] += v[r].d[q];
        }
    }
    const int lane = threadIdx.x & (MCX_WAVE - 1), w = threadIdx.x / MCX_WAVE;
#pragma unroll
    for (int k = 0; k < KTX_N; ++k) {
        const double t = wave_sum(acc[k]);
        if (lane == 0) wsum[w][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < KTX_N) {
        double t = 0.0;
        for (int q = 0; q < MCX_BLOCK / MCX_WAVE; ++q) t += wsum[q][threadIdx.x];
        a.partials[(int64_t)blockIdx.x * KTX_N + threadIdx.x] = t;
    }
}

// ---- FVA with tangents: the dual of k4_fva (k4_fva.hip) -------------------------------------------------------------------------
// Per path, c the counterparty, o the own name, x_m the dual unsecured exposure and the sums over m = 0 .. n_dates-2:
//   w = S_c(0,t_m) S_o(0,t_m)      fca = sum pos(x_m) (w phi_b(m))      fba = sum neg(x_m) (w phi_l(m))      fva = fca - fba
// pos / neg as kt_xva (torch.relu: both legs zero in every image at x.v == 0, the closed threshold band included).  A name without
// atoms is the dual constant 1 (wave-uniform test).  The weights phi are constants of the model parameters: plain doubles without a
// tangent, read wave-uniformly (scalar loads) from a staged table, as k4_fva reads them.
// The products are the Dual operators of mcx_dual.h, not explicit fma: under -ffp-contract=on a tangent a.d b.v + a.v b.d contracts
// inside the operator, but the product of a summand and its addition to the accumulator are two statements and stay two roundings
// (k4_fva's value leg is one fma: the two value images agree to a rounding per date, not bit for bit).  The association is k4_fva's
// (w, then w phi, then times the leg), so swapping the two weight tables and negating every exposure image runs the same arithmetic
// on the other accumulator; with no names and unit weights every product is exact and fca is the sequential sum of pos(x_m), image
// by image.  fva is the difference of the two finished legs in a statement of its own.
// Launch shape and reduction: those of kt_xva (a lane owns a path with a grid stride; wave_sum, a [4 waves][15] table in LDS, 480 B,
// behind ONE barrier; one partial per block, no float atomics).
#define KTV_R 3                                  // records: fca, fba, fva (FVAMetric.EVALUATIONS)
#define KTV_N (KTV_R * (1 + NP))                 // sums per block: [record][image]
// blocks of one launch.  The kernel holds 4 waves per SIMD (profiles/fva_tangent_resource_usage.txt), i.e. 4 blocks of 4 waves per
// CU: 4 x 256 CUs of the MI355X fill every wave slot the kernel can hold in ONE round; more paths than 1024 x 256 take the grid
// stride.  A constant, as KT_XVA_GRID_CAP: the sums of a book do not depend on the device's size
constexpr int KT_FVA_GRID_CAP = 1024;
// the partials of a full grid fit the handle's workspace and its pinned buffer: mcx_tangent_fva's workspace refusal cannot be reached
static_assert(sizeof(double) * KT_FVA_GRID_CAP * KTV_N <= MCX_WS_BYTES && sizeof(double) * KT_FVA_GRID_CAP * KTV_N <= MCX_PINNED_BYTES,
              "kt_fva: the block partials of a full grid exceed the handle's workspace or pinned buffer");

struct KTVArgs {
    KTBook b;
    const double* __restrict__ expo;           // [1+NP][n_rows][ld] of ONE netting set (stride ex_stride between tangents)
    const int32_t* __restrict__ rows;
    const int32_t* __restrict__ delayed;
    const int32_t* __restrict__ surv_c;        // device [n_dates-1] atom ids of S_c(0,t_m), or nullptr: the counterparty never defaults
    const int32_t* __restrict__ surv_o;        // the same for the own name
    const double* __restrict__ w_borrow;       // device [n_dates-1]
    const double* __restrict__ w_lend;
    double* __restrict__ partials;             // [gridDim.x][KTV_R][1+NP]
    int64_t ex_stride;
    double threshold;
    int32_t n_dates, collateralized;
};

__global__ __launch_bounds__(MCX_BLOCK) void kt_fva(const KTVArgs a)
{
    __shared__ double wsum[MCX_BLOCK / MCX_WAVE][KTV_N];
    double acc[KTV_N];
#pragma unroll
    for (int k = 0; k < KTV_N; ++k) acc[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x; i < a.b.n; i += (int64_t)gridDim.x * MCX_BLOCK) {
        DN fca = dconst<NP>(0.0), fba = dconst<NP>(0.0);
        for (int m = 0; m < a.n_dates - 1; ++m) {
            const DN x = kt_unsecured(a.expo, a.ex_stride, a.rows, a.delayed, a.collateralized, a.threshold, a.b.ld, m, i);
            DN ep = dconst<NP>(0.0), en = dconst<NP>(0.0);          // relu: the gradient passes where the leg is strictly positive
            if (x.v > 0.0) ep = x;
            else if (x.v < 0.0) en = 0.0 - x;
            DN Sc = dconst<NP>(1.0), So = dconst<NP>(1.0);
            if (a.surv_c) {                                         // wave-uniform tests
                const int sa = ldk(a.surv_c + m);
                Sc = kt_atom(a.b, ldk_struct(&a.b.atoms[sa]), sa, i);
            }
            if (a.surv_o) {
                const int sa = ldk(a.surv_o + m);
                So = kt_atom(a.b, ldk_struct(&a.b.atoms[sa]), sa, i);
            }
            const DN w = Sc * So;
            const DN wb = w * ldk(a.w_borrow + m), wl = w * ldk(a.w_lend + m);
            fca = fca + ep * wb;
            fba = fba + en * wl;
        }
        const DN fva = fca - fba;
        acc[0] += fca.v; acc[1 + NP] += fba.v; acc[2 * (1 + NP)] += fva.v;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            acc[1 + q] += fca.d[q];
            acc[(1 + NP) + 1 + q] += fba.d[q];
            acc[2 * (1 + NP) + 1 + q] += fva.d[q];
        }
    }
    const int lane = threadIdx.x & (MCX_WAVE - 1), w = threadIdx.x / MCX_WAVE;
#pragma unroll
    for (int k = 0; k < KTV_N; ++k) {
        const double t = wave_sum(acc[k]);
        if (lane == 0) wsum[w][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < KTV_N) {
        double t = 0.0;
        for (int q = 0; q < MCX_BLOCK / MCX_WAVE; ++q) t += wsum[q][threadIdx.x];
        a.partials[(int64_t)blockIdx.x * KTV_N + threadIdx.x] = t;
    }
}

// ---- EPE / ENE profile tangents: sum_i 1[u > 0] du and sum_i 1[u < 0] du per metric date (epe_metric.py, ene_metric.py) -----
struct KTFArgs {
    const double* __restrict__ expo;           // [1+NP][n_rows][ld] of one netting set
    const int32_t* __restrict__ rows;
    const int32_t* __restrict__ delayed;
    double* __restrict__ partials;             // [n_dates][gridDim.x][2*NP]
    int64_t ex_stride, n, ld;
    double threshold;
    int32_t collateralized, pad;
};

__global__ __launch_bounds__(MCX_BLOCK) void kt_profiles(const KTFArgs a)
{
    const int m = blockIdx.y;
    double acc[2 * NP];
#pragma unroll
    for (int q = 0; q < 2 * NP; ++q) acc[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * MCX_BLOCK) {
        const DN u = kt_unsecured(a.expo, a.ex_stride, a.rows, a.delayed, a.collateralized, a.threshold, a.ld, m, i);
        const double wp = u.v > 0.0 ? 1.0 : 0.0, wn = u.v < 0.0 ? 1.0 : 0.0;      // torch.relu: zero gradient at 0
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            acc[q] = fma(wp, u.d[q], acc[q]);
            acc[NP + q] = fma(wn, u.d[q], acc[NP + q]);
        }
    }
    __shared__ double lds[4];
#pragma unroll
    for (int q = 0; q < 2 * NP; ++q) {
        const double r = block_sum(acc[q], lds);
        if (threadIdx.x == 0) a.partials[((int64_t)m * gridDim.x + blockIdx.x) * 2 * NP + q] = r;
    }
}

// ---- PFE tangent: d x_(r) / d theta = the tangent of the path that realises the order statistic (pfe_metric.py:61-66: the
// reference differentiates through torch.sort, i.e. through the selected element) -------------------------------------------
struct KTQArgs {
    const double* __restrict__ expo;
    const int32_t* __restrict__ rows;
    const int32_t* __restrict__ delayed;
    const double* __restrict__ targets;        // [n_dates] exact order statistic of the unsecured exposure (K5 radix select)
    unsigned long long* __restrict__ first;    // [n_dates] smallest local path index with u == target (init: ~0)
    double* __restrict__ out;                  // [n_dates][1+NP]: index (or -1), tangent
    int64_t ex_stride, n, ld;
    double threshold;
    int32_t collateralized, pad;
};

__global__ __launch_bounds__(MCX_BLOCK) void kt_pick_find(const KTQArgs a)
{
    const int m = blockIdx.y;
    const double target = ldk(a.targets + m);
    unsigned long long best = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * MCX_BLOCK) {
        const DN u = kt_unsecured(a.expo, a.ex_stride, a.rows, a.delayed, a.collateralized, a.threshold, a.ld, m, i);
        if (u.v == target && (unsigned long long)i < best) best = (unsigned long long)i;
    }
    if (best != ~0ull) atomicMin(a.first + m, best);
}

__global__ void kt_pick_read(const KTQArgs a, int n_dates)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_dates) return;
    const unsigned long long i = a.first[m];
    double* o = a.out + (int64_t)m * (1 + NP);
    if (i == ~0ull) {
        o[0] = -1.0;
        for (int q = 0; q < NP; ++q) o[1 + q] = 0.0;
        return;
    }
    const DN u = kt_unsecured(a.expo, a.ex_stride, a.rows, a.delayed, a.collateralized, a.threshold, a.ld, m, (int64_t)i);
    o[0] = (double)i;
    for (int q = 0; q < NP; ++q) o[1 + q] = u.d[q];
}

template <int NSLOT, int NZ>
void launch_ktp(const KTPArgs& a, int grid, bool inject, hipStream_t s)
{
    if (inject) hipLaunchKernelGGL((kt_paths<NSLOT, NZ, true>), dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((kt_paths<NSLOT, NZ, false>), dim3(grid), dim3(MCX_BLOCK), 0, s, a);
}
template <int NSLOT, int NZ>
void launch_ktp_chol(const KTPCholArgs& a, int grid, bool inject, hipStream_t s)
{
    if (inject) hipLaunchKernelGGL((kt_paths_chol<NSLOT, NZ, true>), dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((kt_paths_chol<NSLOT, NZ, false>), dim3(grid), dim3(MCX_BLOCK), 0, s, a);
}

// the book's device tables (the id tables are uploaded by the first call that gets here) and the call's dual tensors
int fill_book(mcx_handle* h, const mcx_book* b, const double* d_datoms, const double* d_paths, const double* d_dpaths, int64_t n_paths,
              int64_t ld, int32_t n_dates, KTBook* out)
{
    if (int rc = mcx_book_tangent_ids(h, b)) return rc;
    out->terms = b->d_terms; out->events = b->d_events; out->atoms = b->d_atoms; out->ev_ids = b->d_event_ids; out->term_atom = b->d_term_atom;
    out->datoms = d_datoms; out->paths = d_paths; out->dpaths = d_dpaths; out->n = n_paths; out->ld = ld;
    out->pstride = (int64_t)n_dates * b->n_state * ld; out->n_state = b->n_state; out->n_basis = b->n_basis;
    return 0;
}

// does event e have a tangent form?  `allowed`: the kinds the caller's kernel handles, one bit (1 << MCX_EV_*) each.  Of those,
// options in plain mode — in the payoff modes 1-5 where the caller's kernel has them AND the book is armed with their host tangents
// (KT_PAYOFF_MODES; mcx_book_set_payoff_tangents) — and exercise events under the Bermudan (0) or FlexiCall (1) rule, neither over
// per-term denominators (kt_term_sum's `own` is read by CASHFLOW events only).  The callers word their own messages.
enum KTForm { KT_FORM_OK = 0, KT_FORM_NONE, KT_FORM_TERM_DEN };
constexpr unsigned KT_CASH_KINDS = 1u << MCX_EV_CASHFLOW | 1u << MCX_EV_OPTION;
constexpr unsigned KT_PAYOFF_MODES = 1u << 31;
bool kt_payoff_mode(const DevEvent& e) { return e.kind == MCX_EV_OPTION && e.aux[0] != 0.0; }
KTForm kt_tangent_form(const mcx_book* b, const DevEvent& e, unsigned allowed)
{
    if (e.kind < 0 || e.kind > MCX_EV_EXPO_BS || !(allowed >> e.kind & 1u)) return KT_FORM_NONE;
    if (kt_payoff_mode(e)) {
        const bool known = e.aux[0] == 1.0 || e.aux[0] == 2.0 || e.aux[0] == 3.0 || e.aux[0] == 4.0 || e.aux[0] == 5.0;
        if (!((allowed & KT_PAYOFF_MODES) && b->d_dpayoff && known)) return KT_FORM_NONE;
    }
    if (e.kind == MCX_EV_EXERCISE && e.aux[0] != 0.0 && e.aux[0] != 1.0) return KT_FORM_NONE;
    if (e.kind == MCX_EV_OPTION || e.kind == MCX_EV_EXERCISE)
        for (int j = e.term_begin; j < e.term_end; ++j)
            if (b->h_terms[j].den >= 0) return KT_FORM_TERM_DEN;
    return KT_FORM_OK;
}
// the check of the events [q0, q1) of a moment entry point, which names the option mode in its message
int kt_check_cash_events(mcx_handle* h, const mcx_book* b, int q0, int q1, unsigned allowed, const char* who)
{
    for (int q = q0; q < q1; ++q) {
        const DevEvent& e = b->h_events[q];
        const KTForm f = kt_tangent_form(b, e, allowed);
        if (f == KT_FORM_NONE) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: event %d (kind %d, mode %g) has no tangent form", who, q, e.kind, e.aux[0]);
        if (f == KT_FORM_TERM_DEN) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: option over per-term denominators", who);
    }
    return 0;
}

// what mcx_tangent_lsm and mcx_tangent_lsm_batch check of one (product, regression date) before anything is enqueued; fills the
// device record of the job
int ktl_check_job(mcx_handle* h, const mcx_book* b, const mcx_tangent_lsm_job& q, const char* who, KTLJob* out)
{
    if (q.product < 0 || q.product >= b->n_products) MCX_FAIL(h, -2, "%s: product out of range", who);
    const DevProduct& pr = b->h_products[q.product];
    if (pr.n_states != 1) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: stateless products only", who);
    const int n_cf = pr.cf_end - pr.cf_begin;
    if (q.first_event < 0 || q.first_event > n_cf) MCX_FAIL(h, -2, "%s: first_event out of range", who);
    if (int rc = kt_check_cash_events(h, b, pr.cf_begin, pr.cf_end, KT_CASH_KINDS | KT_PAYOFF_MODES, who)) return rc;
    if (q.num_atom < 0 || q.num_atom >= b->n_atoms || q.x_atom < 0 || q.x_atom >= b->n_atoms) MCX_FAIL(h, -2, "%s: atom out of range", who);
    memset(out, 0, sizeof(*out));
    out->num = mcx_flat_atom(b->h_atoms[q.num_atom]); out->x = mcx_flat_atom(b->h_atoms[q.x_atom]); out->num_id = q.num_atom; out->x_id = q.x_atom;
    out->shift = q.shift; out->scale = q.scale; out->ev_first = pr.cf_begin + q.first_event; out->ev_end = pr.cf_end;
    return 0;
}

// upper bound (bytes) of the partial sums of one kt_lsm_batch launch: the handle's workspace, or less where
// MCX_TANGENT_BATCH_PARTIAL_BYTES says so (include/mcx.h; unset or unparsable: the workspace).  A launch always takes at least one job.
size_t ktl_partial_cap(const mcx_handle* h)
{
    size_t cap = h->ws_bytes;
    const char* e = getenv("MCX_TANGENT_BATCH_PARTIAL_BYTES");
    if (e && *e) {
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end != e && *end == 0 && v > 0 && (size_t)v < cap) cap = (size_t)v;
    }
    return cap;
}
constexpr int KTL_MAX_LAUNCH_JOBS = 32768;     // gridDim.y

// mcx_tangent_lsm_batch, and mcx_tangent_lsm as its one-job case (`who`; the batch names the job in front of a job's refusal).
// Every job of the table in launches of grid (tiles, jobs): the job table (scratch slot 1 where the ring is too small) and the
// result block (slot 3) exist once per call; partials [job][tile][1+NP][NM] in the workspace, as many whole jobs per launch as
// fit; ONE synchronisation, at the end
int ktl_run(mcx_handle* h, const mcx_book* b, const mcx_tangent_lsm_job* h_jobs, int32_t n_jobs, const double* d_datoms, const double* d_paths,
            const double* d_dpaths, int64_t n_paths, int64_t ld, int32_t n_dates, double* h_moments, hipStream_t s, const char* who, bool name_job)
{
    if (ld < n_paths) MCX_FAIL(h, -2, "%s: ld < n_paths", who);
    const int K = b->n_basis, NM = (2 * K - 1) + K, count = (1 + NP) * NM;
    std::vector<KTLJob> jobs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j)
        if (int rc = ktl_check_job(h, b, h_jobs[j], who, &jobs[j])) {
            if (name_job) h->err = "job " + std::to_string(j) + ": " + h->err;
            return rc;
        }
    if (K < 1 || K > 4) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: basis size %d has no instantiation", who, K);
    const size_t out_bytes = sizeof(double) * (size_t)n_jobs * count;
    if (n_paths <= 0) { memset(h_moments, 0, out_bytes); return 0; }
    const int tiles = mcx_grid_for(n_paths, MCX_BLOCK, 2 * h->n_cu);       // of every job, whatever the split
    const size_t job_bytes = sizeof(double) * (size_t)tiles * count;
    if (job_bytes > h->ws_bytes) MCX_FAIL(h, -2, "%s: workspace too small", who);
    size_t per_launch = ktl_partial_cap(h) / job_bytes;
    if (per_launch < 1) per_launch = 1;
    if (per_launch > (size_t)KTL_MAX_LAUNCH_JOBS) per_launch = KTL_MAX_LAUNCH_JOBS;
    KTLBatchArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = fill_book(h, b, d_datoms, d_paths, d_dpaths, n_paths, ld, n_dates, &a.b)) return rc;
    const KTLJob* d_jobs = (const KTLJob*)mcx_upload_table(h, 1, jobs.data(), sizeof(KTLJob) * jobs.size(), s);
    double* d_out = (double*)mcx_scratch(h, 3, out_bytes);
    if (!d_jobs || !d_out) return -100;
    a.partials = h->d_ws;
    // the payoff forms are compiled into a second instantiation, taken only when an event some job visits holds one
    bool exotic = false;
    for (int j = 0; j < n_jobs && !exotic; ++j)
        for (int q = jobs[j].ev_first; q < jobs[j].ev_end && !exotic; ++q) exotic = kt_payoff_mode(b->h_events[q]);
    KTWithPayoff<KTLBatchArgs> ax;
    memset(&ax, 0, sizeof(ax));
    ax.px.coeffs = b->d_coeffs; ax.px.dpayoff = b->d_dpayoff; ax.px.bridge = b->d_bridge;
    int rc = 0;
    for (size_t j0 = 0; j0 < (size_t)n_jobs && rc == 0; j0 += per_launch) {
        const size_t nj = std::min(per_launch, (size_t)n_jobs - j0);
        a.jobs = d_jobs + j0;
        ax.a = a;
        if (exotic) { MCX_DISPATCH(KK, K, 4, hipLaunchKernelGGL((kt_lsm_batch<KK, true>), dim3((unsigned)tiles, (unsigned)nj), dim3(MCX_BLOCK), 0, s, ax)); }
        else { MCX_DISPATCH(KK, K, 4, hipLaunchKernelGGL((kt_lsm_batch<KK, false>), dim3((unsigned)tiles, (unsigned)nj), dim3(MCX_BLOCK), 0, s, a)); }
        rc = mcx_sum_partials(h, h->d_ws, (int)nj, tiles, count, d_out + j0 * count, s);
    }
    // the stream is drained before returning, also after a failed launch; h_moments is written by the one copy only
    hipError_t err = rc == 0 ? hipMemcpyAsync(h_moments, d_out, out_bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    const hipError_t sync = hipStreamSynchronize(s);
    if (rc) return rc;
    MCX_HIP(h, err);
    MCX_HIP(h, sync);
    return 0;
}

// the row tables of a metric call (exposure row; delayed row, or none) into its kernel arguments: false + handle error on failure
template <class Args>
bool kt_upload_rows(mcx_handle* h, const int32_t* h_rows, const int32_t* h_delayed, int32_t n, Args* a, hipStream_t s)
{
    a->rows = (const int32_t*)mcx_upload_table(h, 0, h_rows, sizeof(int32_t) * (size_t)n, s);
    a->delayed = h_delayed ? (const int32_t*)mcx_upload_table(h, 1, h_delayed, sizeof(int32_t) * (size_t)n, s) : nullptr;
    return a->rows && (a->delayed || !h_delayed);
}

// the survival / conditional-survival atom ids of one name, [n] each, against the book (mcx_tangent_cva, mcx_tangent_xva)
int kt_check_name_atoms(mcx_handle* h, const mcx_book* b, const char* who, const int32_t* h_surv, const int32_t* h_cond, int n)
{
    for (int m = 0; m < n; ++m)
        if (h_surv[m] < 0 || h_surv[m] >= b->n_atoms || h_cond[m] < 0 || h_cond[m] >= b->n_atoms) MCX_FAIL(h, -2, "%s: atom out of range", who);
    return 0;
}

// mcx_tangent_paths and mcx_tangent_paths_chol.  `chol_entry`: the latter, which also takes the ANALYTICAL scheme of Black-Scholes /
// Vasicek slots with the tangent of the factors (h_dchol).  Every check comes before the first upload: a refused call enqueues nothing
int ktp_paths(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux, const double* h_dchol,
              uint64_t seed, uint64_t path_offset, int64_t n_paths, double* d_paths, double* d_dpaths, int64_t ld, const double* d_inject_z,
              void* stream, const char* who, bool chol_entry)
{
    if (int rc = mcx_tangent_check_args(h, sim, h_dslot, h_dinit, h_daux, h_dchol, chol_entry ? 1u << MCX_SCHEME_ANALYTICAL : 0u, d_paths,
                                        d_dpaths, n_paths, ld, who, false, "mcx_tangent_paths / mcx_tangent_paths_chol"))
        return rc > 0 ? 0 : rc;
    const mcx_sim_desc& sd = sim->desc;
    const bool analytic = chol_entry && sd.scheme == MCX_SCHEME_ANALYTICAL;
    if (sd.scheme != MCX_SCHEME_EULER && !analytic)
        MCX_FAIL(h, MCX_E_NOT_FUSABLE, chol_entry ? "%s: scheme %d: EULER or ANALYTICAL scheme only" : "%s: EULER scheme only", who, (int)sd.scheme);
    if (int rc = mcx_tangent_check_kinds(h, who, sd.slots, sd.n_slots, analytic, false, nullptr)) return rc;
    if (sd.n_z != sd.n_slots) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: one normal per slot expected", who);
    if (sd.n_slots < 1 || sd.n_slots > 4) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: %d slots have no instantiation", who, sd.n_slots);
    if (analytic)                                         // the kernel indexes h_dchol by the steps' factor index
        if (int rc = mcx_tangent_check_steps(h, who, sim, sd.n_chol, false)) return rc;
    hipStream_t s = (hipStream_t)stream;
    KTPCholArgs ac;
    memset(&ac, 0, sizeof(ac));
    KTPArgs& a = ac.p;
    mcx_fill_k1_args(sim, seed, path_offset, n_paths, ld, d_paths, d_inject_z, nullptr, &a.k1);
    mcx_tangent_tables t;
    if (int rc = mcx_tangent_upload(h, sd, h_dslot, h_dinit, h_daux, analytic ? h_dchol : nullptr, s, &t)) return rc;
    a.dslot = t.dslot; a.dinit = t.dinit; a.daux = t.daux; ac.dchol = t.dchol;
    a.dpaths = d_dpaths; a.pstride = (int64_t)sd.n_dates * sd.n_state * ld; a.n_slots = sd.n_slots;
    const int grid = (int)((n_paths + MCX_BLOCK - 1) / MCX_BLOCK);
    const bool inj = d_inject_z != nullptr;
    if (analytic) { MCX_DISPATCH(NS, sd.n_slots, 4, launch_ktp_chol<NS, NS>(ac, grid, inj, s)); }
    else { MCX_DISPATCH(NS, sd.n_slots, 4, launch_ktp<NS, NS>(a, grid, inj, s)); }
    MCX_HIP(h, hipGetLastError());
    MCX_HIP(h, hipStreamSynchronize(s));
    return 0;
}

}  // namespace

// ---- shared by the dual path entry points of kt_book.hip, kt_storage.hip and kt_wide.hip (mcx_internal.h) ----------------------
int mcx_tangent_check_args(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux,
                           const double* h_dchol, unsigned dchol_schemes, const double* d_paths, const double* d_dpaths, int64_t n_paths,
                           int64_t ld, const char* who, bool wide_entry, const char* narrow_who)
{
    if (!h || !sim || !h_dslot || !h_dinit || !h_daux || !d_paths || !d_dpaths) return -1;
    if (wide_entry) {
        if (!sim->wide)
            MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: a narrow sim (mcx_sim_create) goes to mcx_tangent_paths / mcx_tangent_paths_chol; this entry "
                     "point takes a wide sim (mcx_sim_create_wide)", who);
    } else MCX_REFUSE_WIDE(h, sim, narrow_who);
    const int sc = sim->desc.scheme;
    if (!h_dchol && sc >= 0 && sc < 32 && (dchol_schemes >> sc & 1u)) return -1;
    if (n_paths <= 0) return 1;
    if (ld < n_paths) MCX_FAIL(h, -2, "%s: ld < n_paths", who);
    return 0;
}

int mcx_tangent_check_kinds(mcx_handle* h, const char* who, const mcx_slot* slots, int n_slots, bool analytic, bool allow_hw, bool* has_hw)
{
    if (has_hw) *has_hw = false;
    for (int s = 0; s < n_slots; ++s) {
        const int kd = slots[s].kind;
        if (allow_hw && kd == MCX_MODEL_HW) {
            if (has_hw) *has_hw = true;
            continue;
        }
        if (analytic) {
            if (kd != MCX_MODEL_BS && kd != MCX_MODEL_VASICEK)
                MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: slot %d: model kind %d has no analytic tangent step", who, s, kd);
        } else if (kd != MCX_MODEL_BS && kd != MCX_MODEL_VASICEK && kd != MCX_MODEL_CIRPP && kd != MCX_MODEL_CIRPP_DET)
            MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: slot %d: model kind %d has no tangent step", who, s, kd);
    }
    return 0;
}

int mcx_tangent_check_steps(mcx_handle* h, const char* who, const mcx_sim* sim, int n_factors, bool stores)
{
    const mcx_sim_desc& sd = sim->desc;
    if (sd.n_chol < 1) MCX_FAIL(h, -2, "%s: no Cholesky factor", who);
    for (int k = 0; k < sd.n_steps; ++k) {
        const mcx_step& sp = sim->h_steps[k];
        const bool factor_ok = sp.chol_idx >= 0 && sp.chol_idx < n_factors;
        if (!stores && !factor_ok) MCX_FAIL(h, -2, "%s: step %d: factor out of range", who, k);
        if (stores && (!factor_ok || sp.store_idx >= sd.n_dates)) MCX_FAIL(h, -2, "%s: step %d out of range", who, k);
    }
    return 0;
}

int mcx_tangent_upload(mcx_handle* h, const mcx_sim_desc& sd, const double* h_dslot, const double* h_dinit, const double* h_daux,
                       const double* h_dchol, hipStream_t s, mcx_tangent_tables* out)
{
    const size_t row = sizeof(double) * NP;
    out->dslot = (const double*)mcx_upload_table(h, 0, h_dslot, row * sd.n_slots * MCX_SLOT_NPARAM, s);
    out->dinit = (const double*)mcx_upload_table(h, 1, h_dinit, row * sd.n_state, s);
    out->daux = (const double*)mcx_upload_table(h, 2, h_daux, row * sd.n_steps * sd.n_slots * MCX_AUX, s);
    if (!out->dslot || !out->dinit || !out->daux) return -100;
    out->dchol = h_dchol ? (const double*)mcx_upload_table(h, 3, h_dchol, row * sd.n_chol * sd.n_z * sd.n_z, s) : nullptr;
    return h_dchol && !out->dchol ? -100 : 0;
}

extern "C" int mcx_tangent_paths(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux,
                                 uint64_t seed, uint64_t path_offset, int64_t n_paths, double* d_paths, double* d_dpaths, int64_t ld,
                                 const double* d_inject_z, void* stream)
{
    return ktp_paths(h, sim, h_dslot, h_dinit, h_daux, nullptr, seed, path_offset, n_paths, d_paths, d_dpaths, ld, d_inject_z, stream,
                     "mcx_tangent_paths", false);
}

extern "C" int mcx_tangent_paths_chol(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux,
                                      const double* h_dchol, uint64_t seed, uint64_t path_offset, int64_t n_paths, double* d_paths,
                                      double* d_dpaths, int64_t ld, const double* d_inject_z, void* stream)
{
    return ktp_paths(h, sim, h_dslot, h_dinit, h_daux, h_dchol, seed, path_offset, n_paths, d_paths, d_dpaths, ld, d_inject_z, stream,
                     "mcx_tangent_paths_chol", true);
}

// every check comes before the first upload: a refused call enqueues nothing and writes nothing
extern "C" int mcx_tangent_paths_heston(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux,
                                        const double* h_dchol, uint64_t seed, uint64_t path_offset, int64_t n_paths, double* d_paths,
                                        double* d_dpaths, int64_t ld, const double* d_inject_z, const double* d_inject_u, void* stream)
{
    const char* who = "mcx_tangent_paths_heston";
    if (int rc = mcx_tangent_check_args(h, sim, h_dslot, h_dinit, h_daux, h_dchol, 1u << MCX_SCHEME_EULER, d_paths, d_dpaths, n_paths, ld, who,
                                        false, who))
        return rc > 0 ? 0 : rc;
    const mcx_sim_desc& sd = sim->desc;
    const bool euler = sd.scheme == MCX_SCHEME_EULER, qe = sd.scheme == MCX_SCHEME_QE;
    if (sd.n_slots != 1 || sd.slots[0].kind != MCX_MODEL_HESTON || sd.n_z != 2 || sd.n_state != 2 || sd.slots[0].state_off != 0)
        MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: a single Heston slot expected (%d slots, slot 0 of model kind %d)", who, (int)sd.n_slots,
                 sd.n_slots > 0 ? (int)sd.slots[0].kind : 0);
    if (!euler && !qe) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: scheme %d: EULER or QE scheme only", who, (int)sd.scheme);
    if (qe && sd.n_uniform != 1) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: one uniform per sub-step expected under QE", who);
    if (qe && d_inject_z && !d_inject_u) MCX_FAIL(h, -3, "%s: inject_u required with inject_z under QE", who);
    // the kernel reads factor 0 (one factor per EULER / QE run) and stores by store_idx
    if (int rc = mcx_tangent_check_steps(h, who, sim, 1, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    KTPCholArgs ac;
    memset(&ac, 0, sizeof(ac));
    KTPArgs& a = ac.p;
    mcx_fill_k1_args(sim, seed, path_offset, n_paths, ld, d_paths, d_inject_z, d_inject_u, &a.k1);
    mcx_tangent_tables t;
    if (int rc = mcx_tangent_upload(h, sd, h_dslot, h_dinit, h_daux, euler ? h_dchol : nullptr, s, &t)) return rc;
    a.dslot = t.dslot; a.dinit = t.dinit; a.daux = t.daux; ac.dchol = t.dchol;
    a.dpaths = d_dpaths; a.pstride = (int64_t)sd.n_dates * 2 * ld; a.n_slots = 1;
    const int grid = (int)((n_paths + MCX_BLOCK - 1) / MCX_BLOCK);
    const bool inj = d_inject_z != nullptr;
    if (qe && inj) hipLaunchKernelGGL((kt_paths_heston<true, true>), dim3(grid), dim3(MCX_BLOCK), 0, s, ac);
    else if (qe) hipLaunchKernelGGL((kt_paths_heston<true, false>), dim3(grid), dim3(MCX_BLOCK), 0, s, ac);
    else if (inj) hipLaunchKernelGGL((kt_paths_heston<false, true>), dim3(grid), dim3(MCX_BLOCK), 0, s, ac);
    else hipLaunchKernelGGL((kt_paths_heston<false, false>), dim3(grid), dim3(MCX_BLOCK), 0, s, ac);
    MCX_HIP(h, hipGetLastError());
    MCX_HIP(h, hipStreamSynchronize(s));
    return 0;
}

extern "C" int mcx_tangent_lsm(mcx_handle* h, const mcx_book* b, int32_t product, int32_t first_event, int32_t num_atom, int32_t x_atom,
                               double shift, double scale, const double* d_datoms, const double* d_paths, const double* d_dpaths,
                               int64_t n_paths, int64_t ld, int32_t n_dates, double* h_moments, void* stream)
{
    if (!h || !b || !d_datoms || !d_paths || !d_dpaths || !h_moments) return -1;
    const mcx_tangent_lsm_job job = {product, first_event, num_atom, x_atom, shift, scale};
    return ktl_run(h, b, &job, 1, d_datoms, d_paths, d_dpaths, n_paths, ld, n_dates, h_moments, (hipStream_t)stream, "mcx_tangent_lsm", false);
}

extern "C" int mcx_tangent_lsm_batch(mcx_handle* h, const mcx_book* b, const mcx_tangent_lsm_job* h_jobs, int32_t n_jobs,
                                     const double* d_datoms, const double* d_paths, const double* d_dpaths, int64_t n_paths, int64_t ld,
                                     int32_t n_dates, double* h_moments, void* stream)
{
    if (!h || !b || n_jobs < 0) return -1;
    if (n_jobs == 0) return 0;
    if (!h_jobs || !d_datoms || !d_paths || !d_dpaths || !h_moments) return -1;
    return ktl_run(h, b, h_jobs, n_jobs, d_datoms, d_paths, d_dpaths, n_paths, ld, n_dates, h_moments, (hipStream_t)stream, "mcx_tangent_lsm_batch", true);
}

extern "C" int mcx_tangent_lsm_step(mcx_handle* h, const mcx_book* b, int32_t product, int32_t roll_begin, int32_t roll_end, int32_t num_atom,
                                    int32_t x_atom, double shift, double scale, const double* d_datoms, const double* d_paths,
                                    const double* d_dpaths, int64_t n_paths, int64_t ld, int32_t n_dates, double* d_W, double* d_dW,
                                    int64_t ld_w, double* h_moments, void* stream)
{
    const char* who = "mcx_tangent_lsm_step";
    if (!h || !b || !d_datoms || !d_paths || !d_dpaths || !d_W || !d_dW || !h_moments) return -1;
    if (product < 0 || product >= b->n_products) MCX_FAIL(h, -2, "%s: product out of range", who);
    const DevProduct& pr = b->h_products[product];
    const int n_cf = pr.cf_end - pr.cf_begin;
    if (roll_begin < 0 || roll_end < roll_begin || roll_end > n_cf) MCX_FAIL(h, -2, "%s: roll window out of range", who);
    if (ld < n_paths || ld_w < n_paths) MCX_FAIL(h, -2, "%s: leading dimension < n_paths", who);
    if (int rc = kt_check_cash_events(h, b, pr.cf_begin + roll_begin, pr.cf_begin + roll_end, KT_CASH_KINDS | 1u << MCX_EV_EXERCISE, who)) return rc;
    if (num_atom < 0 || num_atom >= b->n_atoms || x_atom < 0 || x_atom >= b->n_atoms) MCX_FAIL(h, -2, "%s: atom out of range", who);
    const int K = b->n_basis, S = pr.n_states, NM = (2 * K - 1) + S * K, count = (1 + NP) * NM;
    if (n_paths <= 0) { memset(h_moments, 0, sizeof(double) * (size_t)count); return 0; }
    hipStream_t s = (hipStream_t)stream;
    const int grid = mcx_grid_for(n_paths, MCX_BLOCK, 2 * h->n_cu);
    KTSArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = fill_book(h, b, d_datoms, d_paths, d_dpaths, n_paths, ld, n_dates, &a.b)) return rc;
    if (!(a.partials = mcx_partials_ws(h, who, grid, count))) return -2;
    a.coeffs = b->d_coeffs; a.W = d_W; a.dW = d_dW; a.ld_w = ld_w; a.w_stride = (int64_t)S * ld_w;
    a.num = mcx_flat_atom(b->h_atoms[num_atom]); a.x = mcx_flat_atom(b->h_atoms[x_atom]); a.num_id = num_atom; a.x_id = x_atom; a.shift = shift; a.scale = scale;
    a.roll_begin = pr.cf_begin + roll_begin; a.roll_end = pr.cf_begin + roll_end;
    bool launched = true;
#define MCX_KTS(KK, SS) hipLaunchKernelGGL((kt_lsm_step<KK, SS>), dim3(grid), dim3(MCX_BLOCK), 0, s, a)
    switch (K * 16 + S) {
    case 2 * 16 + 1: MCX_KTS(2, 1); break;  case 2 * 16 + 2: MCX_KTS(2, 2); break;  case 2 * 16 + 3: MCX_KTS(2, 3); break;
    case 3 * 16 + 1: MCX_KTS(3, 1); break;  case 3 * 16 + 2: MCX_KTS(3, 2); break;  case 3 * 16 + 3: MCX_KTS(3, 3); break;
    case 3 * 16 + 4: MCX_KTS(3, 4); break;  case 4 * 16 + 1: MCX_KTS(4, 1); break;  case 4 * 16 + 2: MCX_KTS(4, 2); break;
    default: launched = false; break;
    }
#undef MCX_KTS
    if (!launched) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: (basis=%d, states=%d) has no instantiation", who, K, S);
    MCX_HIP(h, hipGetLastError());
    return mcx_partials_to_host(h, grid, count, h_moments, s);
}

extern "C" int mcx_tangent_eval(mcx_handle* h, const mcx_book* b, const double* d_datoms, const double* d_coeffs, const double* d_dcoeffs,
                                const double* d_paths, const double* d_dpaths, int64_t n_paths, int64_t ld, int32_t n_dates,
                                double* d_cfs, double* d_expo, const int32_t* h_ev_param, void* stream)
{
    if (!h || !b || !d_datoms || !d_coeffs || !d_dcoeffs || !d_paths || !d_dpaths || !d_cfs || !d_expo) return -1;
    if (n_paths <= 0) return 0;
    bool exotic = false;                                   // an event of a payoff mode: the second instantiation of the kernel
    for (int p = 0; p < b->n_products; ++p) {
        const DevProduct& pr = b->h_products[p];
        const unsigned allowed = KT_CASH_KINDS | KT_PAYOFF_MODES | 1u << MCX_EV_EXPO_POLY | (h_ev_param ? 1u << MCX_EV_EXPO_BS : 0u) |
                                 (pr.n_states > 1 ? 1u << MCX_EV_EXERCISE : 0u);
        for (int q = pr.ev_begin; q < pr.ev_end; ++q) {
            const DevEvent& e = b->h_events[q];
            exotic = exotic || kt_payoff_mode(e);
            const KTForm f = kt_tangent_form(b, e, allowed);
            if (f == KT_FORM_NONE) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "mcx_tangent_eval: event %d (kind %d) has no tangent form", q, e.kind);
            if (f == KT_FORM_TERM_DEN) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "mcx_tangent_eval: option over per-term denominators");
        }
    }
    hipStream_t s = (hipStream_t)stream;
    KTEArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = fill_book(h, b, d_datoms, d_paths, d_dpaths, n_paths, ld, n_dates, &a.b)) return rc;
    if (h_ev_param && !(a.ev_param = (const int32_t*)mcx_upload_table(h, 1, h_ev_param, sizeof(int32_t) * 2 * (size_t)b->n_events, s))) return -100;
    const int n_rows = b->n_expo_rows > 0 ? b->n_expo_rows : 1;
    MCX_HIP(h, hipMemsetAsync(d_cfs, 0, sizeof(double) * (size_t)(1 + NP) * b->n_netting_sets * ld, s));
    MCX_HIP(h, hipMemsetAsync(d_expo, 0, sizeof(double) * (size_t)(1 + NP) * b->n_netting_sets * n_rows * ld, s));
    a.products = b->d_products; a.coeffs = d_coeffs; a.dcoeffs = d_dcoeffs; a.cfs = d_cfs; a.expo = d_expo; a.n_products = b->n_products;
    a.n_ns = b->n_netting_sets; a.n_rows = n_rows;
    const dim3 grid((unsigned)((n_paths + MCX_BLOCK - 1) / MCX_BLOCK));
    if (exotic) {
        KTWithPayoff<KTEArgs> ax;
        memset(&ax, 0, sizeof(ax));
        ax.a = a; ax.px.coeffs = b->d_coeffs; ax.px.dpayoff = b->d_dpayoff; ax.px.bridge = b->d_bridge;
        hipLaunchKernelGGL(kt_eval<true>, grid, dim3(MCX_BLOCK), 0, s, ax);
    } else hipLaunchKernelGGL(kt_eval<false>, grid, dim3(MCX_BLOCK), 0, s, a);
    MCX_HIP(h, hipGetLastError());
    MCX_HIP(h, hipStreamSynchronize(s));
    return 0;
}

extern "C" int mcx_book_set_payoff_tangents(mcx_handle* h, mcx_book* b, const double* d_dpayoff, void* stream)
{
    if (!h || !b) return -1;
    MCX_HIP(h, hipStreamSynchronize((hipStream_t)stream));      // no call in flight reads the rows that are replaced
    b->d_dpayoff = d_dpayoff;
    return 0;
}

extern "C" int mcx_tangent_cva(mcx_handle* h, const mcx_book* b, const double* d_datoms, const int32_t* h_rows, const int32_t* h_surv,
                               const int32_t* h_cond, const int32_t* h_delayed, int32_t collateralized, int32_t n_dates_metric,
                               double threshold, double recovery, const double* d_expo_ns,
                               int64_t expo_tangent_stride, const double* d_paths, const double* d_dpaths, int64_t n_paths, int64_t ld,
                               int32_t n_dates, double* d_out, void* stream)
{
    if (!h || !b || !d_datoms || !h_rows || !h_surv || !h_cond || !d_expo_ns || !d_paths || !d_dpaths || !d_out) return -1;
    if (n_paths <= 0 || n_dates_metric < 1) return 0;
    if (int rc = kt_check_name_atoms(h, b, "mcx_tangent_cva", h_surv, h_cond, n_dates_metric - 1)) return rc;
    hipStream_t s = (hipStream_t)stream;
    KTCArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = fill_book(h, b, d_datoms, d_paths, d_dpaths, n_paths, ld, n_dates, &a.b)) return rc;
    if (!kt_upload_rows(h, h_rows, h_delayed, n_dates_metric, &a, s)) return -100;
    a.surv = (const int32_t*)mcx_upload_table(h, 2, h_surv, sizeof(int32_t) * (size_t)(n_dates_metric - 1), s);
    a.cond = (const int32_t*)mcx_upload_table(h, 3, h_cond, sizeof(int32_t) * (size_t)(n_dates_metric - 1), s);
    if (!a.surv || !a.cond) return -100;
    a.expo = d_expo_ns; a.out = d_out; a.ex_stride = expo_tangent_stride; a.threshold = threshold; a.lgd = 1.0 - recovery;
    a.n_dates = n_dates_metric; a.collateralized = collateralized;
    hipLaunchKernelGGL(kt_cva, dim3((unsigned)((n_paths + MCX_BLOCK - 1) / MCX_BLOCK)), dim3(MCX_BLOCK), 0, s, a);
    MCX_HIP(h, hipGetLastError());
    MCX_HIP(h, hipStreamSynchronize(s));
    return 0;
}

extern "C" int mcx_tangent_xva(mcx_handle* h, const mcx_book* b, const double* d_datoms, const int32_t* h_rows, const int32_t* h_delayed,
                               int32_t collateralized, int32_t n_dates_metric, double threshold,
                               const int32_t* h_surv_c, const int32_t* h_cond_c, double recovery_c,
                               const int32_t* h_surv_o, const int32_t* h_cond_o, double recovery_o,
                               const double* d_expo_ns, int64_t expo_tangent_stride, const double* d_paths, const double* d_dpaths,
                               int64_t n_paths, int64_t ld, int32_t n_dates, double* h_out, void* stream)
{
    const char* who = "mcx_tangent_xva";
    if (!h || !b || !d_datoms || !h_rows || !d_expo_ns || !d_paths || !d_dpaths || !h_out) return -1;
    if (n_paths <= 0 || n_dates_metric <= 1) { memset(h_out, 0, sizeof(double) * KTX_N); return 0; }
    // every check comes before the first upload: a refused call enqueues nothing and leaves h_out as it was
    if (ld < n_paths) MCX_FAIL(h, -2, "%s: leading dimension < n_paths", who);
    if (!h_surv_c != !h_cond_c || !h_surv_o != !h_cond_o)
        MCX_FAIL(h, -2, "%s: the survival and conditional-survival atoms of a name come together (both or neither)", who);
    const int nd = n_dates_metric - 1;
    if (h_surv_c) if (int rc = kt_check_name_atoms(h, b, who, h_surv_c, h_cond_c, nd)) return rc;
    if (h_surv_o) if (int rc = kt_check_name_atoms(h, b, who, h_surv_o, h_cond_o, nd)) return rc;
    for (int m = 0; m < n_dates_metric; ++m)          // the rows index the netting set's exposure block of the book
        if (h_rows[m] < 0 || h_rows[m] >= b->n_expo_rows || (h_delayed && h_delayed[m] >= b->n_expo_rows))
            MCX_FAIL(h, -2, "%s: exposure row of metric date %d out of range", who, m);
    hipStream_t s = (hipStream_t)stream;
    const int grid = mcx_grid_for(n_paths, MCX_BLOCK, KT_XVA_GRID_CAP);
    KTXArgs a;
    memset(&a, 0, sizeof(a));
    const size_t part_bytes = sizeof(double) * (size_t)grid * KTX_N;
    if (part_bytes > h->ws_bytes || part_bytes > h->pinned_bytes) MCX_FAIL(h, -2, "%s: workspace too small", who);
    a.partials = h->d_ws;
    if (int rc = fill_book(h, b, d_datoms, d_paths, d_dpaths, n_paths, ld, n_dates, &a.b)) return rc;
    if (!kt_upload_rows(h, h_rows, h_delayed, n_dates_metric, &a, s)) return -100;
    a.c.lgd = 1.0 - recovery_c; a.o.lgd = 1.0 - recovery_o;
    if (h_surv_c || h_surv_o) {                       // the atom ids of both names in one staged table
        std::vector<int32_t> ids;
        const int32_t* lists[4] = {h_surv_c, h_cond_c, h_surv_o, h_cond_o};
        for (int q = 0; q < 4; ++q)
            if (lists[q]) ids.insert(ids.end(), lists[q], lists[q] + nd);
        const int32_t* d_ids = (const int32_t*)mcx_stage_small(h, ids.data(), sizeof(int32_t) * ids.size(), s);
        if (!d_ids) return -100;
        if (h_surv_c) { a.c.surv = d_ids; a.c.cond = d_ids + nd; d_ids += 2 * nd; }
        if (h_surv_o) { a.o.surv = d_ids; a.o.cond = d_ids + nd; }
    }
    a.expo = d_expo_ns; a.ex_stride = expo_tangent_stride; a.threshold = threshold;
    a.n_dates = n_dates_metric; a.collateralized = collateralized;
    hipLaunchKernelGGL(kt_xva, dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    MCX_HIP(h, hipGetLastError());
    // the block partials (at most 512 x 25 doubles) through the pinned buffer, added in block order on the host as
    // mcx_tangent_profiles adds its own (mcx_partials_to_host's k_sum_partials took 0.124 ms here against the kernel's 0.490 ms at
    // 1,048,576 paths: profiles/xva_tangent_finishing_launch.csv)
    MCX_HIP(h, hipMemcpyAsync(h->h_pinned, a.partials, part_bytes, hipMemcpyDeviceToHost, s));
    MCX_HIP(h, hipStreamSynchronize(s));
    const double* part = (const double*)h->h_pinned;
    double sums[KTX_N] = {};
    for (int q = 0; q < grid; ++q)
        for (int k = 0; k < KTX_N; ++k) sums[k] += part[(size_t)q * KTX_N + k];
    memcpy(h_out, sums, sizeof(sums));
    return 0;
}

extern "C" int mcx_tangent_fva(mcx_handle* h, const mcx_book* b, const double* d_datoms, const int32_t* h_rows, const int32_t* h_delayed,
                               int32_t collateralized, int32_t n_dates_metric, double threshold,
                               const int32_t* h_surv_c, const int32_t* h_surv_o, const double* h_w_borrow, const double* h_w_lend,
                               const double* d_expo_ns, int64_t expo_tangent_stride, const double* d_paths, const double* d_dpaths,
                               int64_t n_paths, int64_t ld, int32_t n_dates, double* h_out, void* stream)
{
    const char* who = "mcx_tangent_fva";
    if (!h) return -1;
    if (!b || !d_datoms || !h_rows || !h_w_borrow || !h_w_lend || !d_expo_ns || !d_paths || !d_dpaths || !h_out)
        MCX_FAIL(h, -1, "%s: a NULL book, buffer, row list, weight table or h_out", who);
    if (n_paths <= 0 || n_dates_metric <= 1) { memset(h_out, 0, sizeof(double) * KTV_N); return 0; }
    // every check comes before the first upload: a refused call enqueues nothing and leaves h_out as it was
    if (ld < n_paths) MCX_FAIL(h, -2, "%s: leading dimension < n_paths", who);
    const int nd = n_dates_metric - 1;
    const int32_t* lists[2] = {h_surv_c, h_surv_o};
    for (int q = 0; q < 2; ++q)
        for (int m = 0; lists[q] && m < nd; ++m)
            if (lists[q][m] < 0 || lists[q][m] >= b->n_atoms) MCX_FAIL(h, -2, "%s: atom out of range", who);
    for (int m = 0; m < n_dates_metric; ++m)          // the rows index the netting set's exposure block of the book
        if (h_rows[m] < 0 || h_rows[m] >= b->n_expo_rows || (h_delayed && h_delayed[m] >= b->n_expo_rows))
            MCX_FAIL(h, -2, "%s: exposure row of metric date %d out of range", who, m);
    hipStream_t s = (hipStream_t)stream;
    const int grid = mcx_grid_for(n_paths, MCX_BLOCK, KT_FVA_GRID_CAP);
    KTVArgs a;
    memset(&a, 0, sizeof(a));
    const size_t part_bytes = sizeof(double) * (size_t)grid * KTV_N;
    if (part_bytes > h->ws_bytes || part_bytes > h->pinned_bytes) MCX_FAIL(h, -2, "%s: workspace too small", who);
    a.partials = h->d_ws;
    if (int rc = fill_book(h, b, d_datoms, d_paths, d_dpaths, n_paths, ld, n_dates, &a.b)) return rc;
    if (!kt_upload_rows(h, h_rows, h_delayed, n_dates_metric, &a, s)) return -100;
    {                                                 // the two weight tables in one staged table, the atom ids in another
        std::vector<double> wts(h_w_borrow, h_w_borrow + nd);
        wts.insert(wts.end(), h_w_lend, h_w_lend + nd);
        const double* d_w = (const double*)mcx_stage_small(h, wts.data(), sizeof(double) * wts.size(), s);
        if (!d_w) return -100;
        a.w_borrow = d_w; a.w_lend = d_w + nd;
    }
    if (h_surv_c || h_surv_o) {
        std::vector<int32_t> ids;
        for (int q = 0; q < 2; ++q)
            if (lists[q]) ids.insert(ids.end(), lists[q], lists[q] + nd);
        const int32_t* d_ids = (const int32_t*)mcx_stage_small(h, ids.data(), sizeof(int32_t) * ids.size(), s);
        if (!d_ids) return -100;
        if (h_surv_c) { a.surv_c = d_ids; d_ids += nd; }
        if (h_surv_o) a.surv_o = d_ids;
    }
    a.expo = d_expo_ns; a.ex_stride = expo_tangent_stride; a.threshold = threshold;
    a.n_dates = n_dates_metric; a.collateralized = collateralized;
    hipLaunchKernelGGL(kt_fva, dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    MCX_HIP(h, hipGetLastError());
    // the block partials (at most KT_FVA_GRID_CAP x 15 doubles) through the pinned buffer, added in block order on the host, as
    // mcx_tangent_xva adds its own
    MCX_HIP(h, hipMemcpyAsync(h->h_pinned, a.partials, part_bytes, hipMemcpyDeviceToHost, s));
    MCX_HIP(h, hipStreamSynchronize(s));
    const double* part = (const double*)h->h_pinned;
    double sums[KTV_N] = {};
    for (int q = 0; q < grid; ++q)
        for (int k = 0; k < KTV_N; ++k) sums[k] += part[(size_t)q * KTV_N + k];
    memcpy(h_out, sums, sizeof(sums));
    return 0;
}

extern "C" int mcx_tangent_profiles(mcx_handle* h, const int32_t* h_rows, const int32_t* h_delayed, int32_t collateralized,
                                    int32_t n_dates_metric, double threshold, const double* d_expo_ns,
                                    int64_t expo_tangent_stride, int64_t n_paths, int64_t ld, double* h_out, void* stream)
{
    if (!h || !h_rows || !d_expo_ns || !h_out) return -1;
    if (n_dates_metric <= 0) return 0;
    memset(h_out, 0, sizeof(double) * (size_t)n_dates_metric * 2 * NP);
    if (n_paths <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int grid = mcx_grid_for(n_paths, MCX_BLOCK, 64);
    std::vector<double> part((size_t)n_dates_metric * grid * 2 * NP);
    KTFArgs a;
    memset(&a, 0, sizeof(a));
    if (!kt_upload_rows(h, h_rows, h_delayed, n_dates_metric, &a, s)) return -100;
    if (!(a.partials = (double*)mcx_scratch(h, 2, sizeof(double) * part.size()))) return -100;
    a.expo = d_expo_ns; a.collateralized = collateralized; a.ex_stride = expo_tangent_stride; a.n = n_paths; a.ld = ld; a.threshold = threshold;
    hipLaunchKernelGGL(kt_profiles, dim3(grid, n_dates_metric), dim3(MCX_BLOCK), 0, s, a);
    MCX_HIP(h, hipGetLastError());
    MCX_HIP(h, hipMemcpyAsync(part.data(), a.partials, sizeof(double) * part.size(), hipMemcpyDeviceToHost, s));
    MCX_HIP(h, hipStreamSynchronize(s));
    for (int m = 0; m < n_dates_metric; ++m)
        for (int b = 0; b < grid; ++b)
            for (int q = 0; q < 2 * NP; ++q) h_out[(size_t)m * 2 * NP + q] += part[((size_t)m * grid + b) * 2 * NP + q];
    return 0;
}

extern "C" int mcx_tangent_pick(mcx_handle* h, const int32_t* h_rows, const int32_t* h_delayed, int32_t collateralized,
                                int32_t n_dates_metric, double threshold, const double* h_targets, const double* d_expo_ns,
                                int64_t expo_tangent_stride, int64_t n_paths, int64_t ld, double* h_out, void* stream)
{
    if (!h || !h_rows || !h_targets || !d_expo_ns || !h_out) return -1;
    if (n_dates_metric <= 0) return 0;
    for (int m = 0; m < n_dates_metric; ++m) { h_out[(size_t)m * (1 + NP)] = -1.0; for (int q = 0; q < NP; ++q) h_out[(size_t)m * (1 + NP) + 1 + q] = 0.0; }
    if (n_paths <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    KTQArgs a;
    memset(&a, 0, sizeof(a));
    if (!kt_upload_rows(h, h_rows, h_delayed, n_dates_metric, &a, s)) return -100;
    a.targets = (const double*)mcx_upload_table(h, 2, h_targets, sizeof(double) * (size_t)n_dates_metric, s);
    // results, slot 3: out [n_dates][1+NP], then first [n_dates]
    const size_t out_bytes = sizeof(double) * (size_t)n_dates_metric * (1 + NP), first_bytes = sizeof(unsigned long long) * (size_t)n_dates_metric;
    a.out = (double*)mcx_scratch(h, 3, out_bytes + first_bytes);
    if (!a.targets || !a.out) return -100;
    a.first = (unsigned long long*)(a.out + (size_t)n_dates_metric * (1 + NP));
    MCX_HIP(h, hipMemsetAsync(a.first, 0xFF, first_bytes, s));
    a.expo = d_expo_ns; a.ex_stride = expo_tangent_stride; a.n = n_paths; a.ld = ld; a.threshold = threshold; a.collateralized = collateralized;
    hipLaunchKernelGGL(kt_pick_find, dim3(mcx_grid_for(n_paths, MCX_BLOCK, 256), n_dates_metric), dim3(MCX_BLOCK), 0, s, a);
    hipLaunchKernelGGL(kt_pick_read, dim3((n_dates_metric + 63) / 64), dim3(64), 0, s, a, n_dates_metric);
    MCX_HIP(h, hipGetLastError());
    MCX_HIP(h, hipMemcpyAsync(h_out, a.out, out_bytes, hipMemcpyDeviceToHost, s));
    MCX_HIP(h, hipStreamSynchronize(s));
    return 0;
}
