// kf_lean.hip — the one-launch main pass for books whose every timeline date compiled to a straight-line FastDate record
// (kf_common.h): Philox + Box-Muller + Cholesky + SDE sub-steps, the date's cashflows / regression exposure / threshold /
// EPE-ENE records / CVA increment, and the block accumulators — nothing materialised in HBM.
//
// Reference dataflow replaced: controller/controller.py:677-694 (generate_paths -> resolve_requests -> evaluate_products ->
// metric reductions) for the linear-book shape (bond.py:115-214, swap.py:129-172 cashflows; controller.py:385-471 exposures;
// cva_metric.py:23-100; epe/ene_metric.py).
//
// Mapping to the hardware (MI355X: 256 CUs x 4 SIMDs, f64 VALU issue is the bound of this kernel — MI355X_MICROARCH.md):
//   * TWO paths per lane (PPL = 2): a lane carries two independent RNG / SDE / payoff dependency chains, so 4 resident
//     waves per SIMD give the issue parallelism of 8 and every wave-uniform cost (scalar table loads, SALU control, the
//     date record) is paid once per 128 paths instead of once per 64;
//   * the launch is sized to the residency the code object guarantees: __launch_bounds__(256, 4) => <= 128 VGPRs, 4 blocks
//     per CU for any SGPR count (800 / (ceil(sgpr/16)*16 + 16) >= 4), so grid = 4 x CUs blocks are all co-resident and the
//     path tiles (512 paths per block-tile) are dealt round-robin: 2^20 paths = 2048 tiles = exactly two rounds, no
//     partially filled last round (the round-1 kernel ran 8 waves per SIMD slot on a 6-7 wave residency: one round in
//     eight at a fraction of the issue rate);
//   * scalar state is REGION-LOCAL: every code region (tile prologue, one run of sub-steps, a date block, tile epilogue)
//     reads the kernel arguments, the FastDate record and the polynomial coefficient tables through a pointer that carries
//     a "region zero" (mcx_math.h), i.e. as scalar loads at the point of use.  Left alone, the backend loads all ~100
//     argument dwords in the prologue, keeps them live through every loop and spills them to VGPR lanes; each reload is a
//     v_readlane — a VALU instruction, the pipe this kernel is bound by (the round-1 kernel carried 82 such spills).
#include <cstdlib>
#include <map>
#include <utility>

#include "kf_common.h"

namespace {

// The CVA-only date of the cva-date instantiation (DK = 1): a Vasicek + CIR++ book whose every date is the merged CVA block
// of lean_date (kf_common.h) or has no effect (FastDateCva, kf_common.h).  The record comes from LDS (staged once per block by the kernel
// prologue) as uniform-address wide reads, so no SGPR is held across the sub-step runs and nothing waits on a chain of scalar
// loads; no flag is decoded; the state registers are compile-time indices (no M0-relative moves); the four exponentials of
// the lane go out as one round of table reads.  Same arithmetic, in the same order, as the merged CVA block of lean_date.
template <int NSLOT, int PPL>
__device__ __forceinline__ void lean_date_cva(const FastDateCvaLds* __restrict__ rp, const double (&reg)[PPL][2 * NSLOT], double (&cva)[PPL],
                                              const double* __restrict__ etab)
{
    const mcx_expq_coef ec = mcx_expq_load(mcx_region_zero());
    const FastDateCvaLds r = *rp;
    double xe[2 * PPL], ev[2 * PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        xe[2 * q] = fma(r.m_s1, reg[q][FDC_S_REG], fma(r.m_n1, reg[q][FDC_NI_REG], r.m_c0));
        xe[2 * q + 1] = fma(r.c_c1, reg[q][FDC_C_REG], r.c_c0);
    }
    mcx_exp_tab_n<2 * PPL>(xe, ev, etab, ec);
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const double x = fma(r.x_d, reg[q][FDC_X_REG], r.x_a);
        double p = 0.0;
        p += fma(fma(r.row0[2], x, r.row0[1]), x, r.row0[0]);
        p += fma(fma(r.row1[2], x, r.row1[1]), x, r.row1[0]);
        const double w = r.m_b * ev[2 * q];
        const double cs = fma(r.c_b, ev[2 * q + 1], r.c_a);
        cva[q] = fma(fmax(p, 0.0), w * (1.0 - cs), cva[q]);
    }
}

// ---- the draws of the cva-date instantiation (DK = 1) ---------------------------------------------------------------------------
// draw_pairs_staged (mcx_device.h) for a launch whose grid is the kernel's whole residency and whose paths share ONE high word of the path index
// (launch_lean_shape checks both) and whose sub-step is the same for every path of the lane: the same bits, less vector work.
// The stages are written as there, but the backend does not keep them: the results of stage C are dead where the rare-draw
// branch is taken, so it sinks the stage behind that branch and waits for the table reads after a few of its instructions.
// Measured at four waves per SIMD, that order is faster than the staged one; thin launches, which the
// staging is for, run DK = 2.
//   * Philox: the counter is (path_lo, path_hi, step, draw) and only path_lo differs between lanes, so all of round 1 but
//     M0 * path_lo, the product M0 * (hi(M1 step) ^ path_hi ^ k0) of round 2 and the key folds of rounds 2 and 3 are wave-uniform:
//     written on scalars, they run on the SALU (a VOP3 reads one SGPR: two scalars are xor-ed before they meet a vector);
//   * the second uniform's remainder from integers, see cva_draw_pairs;
//   * one rare-draw test per lane.
template <int PPL>
__device__ __forceinline__ void philox4x32_10_cva(const uint32_t (&path_lo)[PPL], uint32_t path_hi, uint32_t step, uint32_t draw, uint64_t seed,
                                                  uint32_t (&o0)[PPL], uint32_t (&o1)[PPL], uint32_t (&o2)[PPL], uint32_t (&o3)[PPL])
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t c0[PPL], c1[PPL], c2[PPL], c3[PPL];
    // round 1: c0 and c1 come out scalar, c2 and c3 per lane
    const uint64_t s1 = (uint64_t)M1 * step;
    const uint32_t hk = path_hi ^ k0;
    const uint32_t a0 = (uint32_t)(s1 >> 32) ^ hk, a1 = (uint32_t)s1;
    const uint32_t dk = draw ^ k1;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const uint64_t p0 = (uint64_t)M0 * path_lo[q];
        c2[q] = (uint32_t)(p0 >> 32) ^ dk;
        c3[q] = (uint32_t)p0;
    }
    k0 += W0; k1 += W1;
    // round 2: M0 * c0 is a scalar product and c3 comes out scalar; the round keys are folded into the per-lane words, which do
    // not depend on the sub-step (the keys then need no register of their own inside a run of sub-steps)
    const uint64_t s0 = (uint64_t)M0 * a0;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const uint64_t p1 = (uint64_t)M1 * c2[q];
        c0[q] = ((uint32_t)(p1 >> 32) ^ k0) ^ a1;
        c2[q] = (c3[q] ^ k1) ^ (uint32_t)(s0 >> 32);
        c1[q] = (uint32_t)p1;
    }
    k0 += W0; k1 += W1;
    // round 3: the last scalar word (c3) and its key
    const uint32_t x3 = (uint32_t)s0 ^ k1;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const uint64_t p0 = (uint64_t)M0 * c0[q];
        const uint64_t p1 = (uint64_t)M1 * c2[q];
        c0[q] = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1[q], k0, 0x96);
        c2[q] = (uint32_t)(p0 >> 32) ^ x3;
        c1[q] = (uint32_t)p1; c3[q] = (uint32_t)p0;
    }
    k0 += W0; k1 += W1;
#pragma unroll
    for (int r = 3; r < 10; ++r) {                                      // rounds 4-10: philox4x32_10_n
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const uint64_t p0 = (uint64_t)M0 * c0[q];
            const uint64_t p1 = (uint64_t)M1 * c2[q];
            const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1[q], k0, 0x96);
            const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3[q], k1, 0x96);
            c1[q] = (uint32_t)p1; c3[q] = (uint32_t)p0; c0[q] = n0; c2[q] = n2;
        }
        k0 += W0; k1 += W1;
    }
#pragma unroll
    for (int q = 0; q < PPL; ++q) { o0[q] = c0[q]; o1[q] = c1[q]; o2[q] = c2[q]; o3[q] = c3[q]; }
}

// Constants of the integer-built remainder, kept in VGPRs across a run of sub-steps like the additive ones of mcx_bm_vconst
// (mcx_math.h): the kernel has vector registers to spare and none of the scalar ones
struct CvaDrawConst {
    double off52;          // 2^52 - 1/2
    double trig_scale;     // 2 pi 2^-53
};
__device__ __forceinline__ CvaDrawConst cva_draw_const_make()
{
    CvaDrawConst c;
    c.off52 = mcx_opaque_v(0x1.0p52 - 0.5); c.trig_scale = mcx_opaque_v(6.28318530717958647692 * 0x1.0p-53);
    return c;
}

// The second uniform's remainder ur = (n' + 1/2) 2^-53, n' = (w3 & mask) 2^21 + (w2 >> 11) < 2^(53 - BMB), enters the angle only as
// d = fma(ur, 2 pi, trig_off).  The words (0x43300000 | n' >> 32, n' & 0xffffffff) are the double 2^52 + n'; subtracting 2^52 - 1/2 is
// exact (n' + 1/2 has at most 54 - BMB bits), and (n' + 1/2) (2 pi 2^-53) is the same real product as ur (2 pi): one rounding in the
// fma, the same d.  Three integer operations and an addition replace a shift, two conversions and two fmas.
template <int PPL, int BMB>
__device__ __forceinline__ bool cva_draw_pairs(uint64_t seed, const uint32_t (&path_lo)[PPL], uint32_t path_hi, uint32_t step, uint32_t draw,
                                               double (&z0)[PPL], double (&z1)[PPL], const double* __restrict__ tab,
                                               const mcx_bm_coef& C, const mcx_bm_vconst& vc, const CvaDrawConst& dc)
{
    static_assert(BMB >= 1 && BMB <= 20, "the funnel shift of the high word is by 11 + BMB < 32 bits");
    constexpr int N = 1 << BMB, LOG_TERMS = mcx_bm_shape<BMB>::LOG_TERMS;
    uint32_t w0[PPL], w1[PPL], w2[PPL], w3[PPL];
    philox4x32_10_cva<PPL>(path_lo, path_hi, step, draw, seed, w0, w1, w2, w3);
    double m[PPL], ed[PPL], ps[PPL], pc[PPL];
    int e[PPL];
    mcx_d2 tc[PPL], sc[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {                                     // (B) cells and table reads
        const double ua = u53(w0[q], w1[q], &vc);
        m[q] = __builtin_amdgcn_frexp_mant(ua);
        e[q] = __builtin_amdgcn_frexp_exp(ua);
        const int jl = (__double2hiint(m[q]) >> (20 - BMB)) & (N - 1);
        tc[q] = ((const mcx_d2*)tab)[jl];
        sc[q] = ((const mcx_d2*)(tab + 2 * N))[(int)(w3[q] >> (32 - BMB))];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < PPL; ++q) {                                     // (C) no table value needed
        const uint32_t lo = __builtin_amdgcn_alignbit(w3[q], w2[q], 11);
        // 0x43300000 | (w3 & mask) >> 11 as one funnel shift of the constant over w3 << BMB
        const uint32_t hi = __builtin_amdgcn_alignbit(0x43300000u >> (21 - BMB), w3[q] << BMB, 11 + BMB);
        const double v = __hiloint2double((int)hi, (int)lo) - dc.off52;
        const double d = fma(v, dc.trig_scale, vc.trig_off);
        const double d2 = d * d;
        double qs, qc;
        if constexpr (mcx_bm_shape<BMB>::TRIG_TERMS == 3) {
            qs = fma(fma(vc.sin_head, d2, C.c[7]), d2, C.c[6]);
            qc = fma(fma(vc.cos_head, d2, C.c[10]), d2, C.c[9]);
        } else {
            qs = fma(vc.sin_head, d2, C.c[6]);
            qc = fma(vc.cos_head, d2, C.c[9]);
        }
        ps[q] = fma(d * d2, qs, d);
        pc[q] = fma(d2, qc, 1.0);
        ed[q] = (double)e[q];
    }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t top = 0;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {                                     // (D) radius and rotation
        const double s = fma(m[q], tc[q].x, 2.0);
        double p = vc.log_head;
#pragma unroll
        for (int k = LOG_TERMS - 2; k >= 0; --k) p = fma(p, s, C.c[k]);
        const double r2 = fma(ed[q], -2.0 * 6.93147180559945309417e-01, tc[q].y) + fma(s * s, p, s);
        const double r = mcx_sqrt_gp(r2);
        const double sn = fma(sc[q].x, pc[q], sc[q].y * ps[q]);
        const double cs = fma(-sc[q].x, ps[q], sc[q].y * pc[q]);
        z0[q] = r * cs;
        z1[q] = r * sn;
        top = w1[q] > top ? w1[q] : top;
    }
    // a first uniform may round to 1 only where its high word is all ones: the largest of the lane's high words is all ones exactly
    // when one of them is (one v_max_u32 and one compare; the AND of the words would miss a lane that holds a single such word)
    return top == 0xffffffffu;
}

#define MCX_LEAN_WAVES 4
// SIMULATE = false: the same date programs on a paths tensor produced earlier by K1 (k1.paths is then the INPUT
// [date][state][path]): one streaming pass, the next date's state columns in flight while this date's program runs
// (Measured and dropped: drawing the normals of 2-5 sub-steps AHEAD as independent staged chains, for small path counts — the draws
// depend on the counter (path, step) only.  No gain at one or two waves per SIMD: what a thin launch waits for is scalar work, see
// launch_lean.)
// DK (date kind) != 0: every date through lean_date_cva from the FastDateCvaLds records that follow the record area in the
// dynamic LDS (launch_lean_shape: a.cva_dates != nullptr).  DK = 1 draws through cva_draw_pairs: the kernel of a launch whose grid is
// the whole residency.  DK = 2 keeps draw_pairs_staged: the kernel of a thin launch (one or two waves per SIMD), see launch_lean_shape.
template <int NSLOT, int NZ, bool INJECT, int SIG, int PPL, bool SIMULATE, int DK = 0>
__global__ __launch_bounds__(MCX_BLOCK, MCX_LEAN_WAVES) void kf_lean(const FusedArgs)      // read through kargs_region(), never by name
{
    static_assert(DK == 0 || (SIG == SIG_VAS_CIR_E && SIMULATE && !INJECT), "the cva-date kernel simulates the Vasicek + CIR++ signature");
    constexpr int NREG = 2 * NSLOT;
    constexpr int TILE = MCX_BLOCK * PPL;
    extern __shared__ double lds[];
    KArgs& a0 = kargs_region(0);
    const int n_rec = a0.n_rec;
    const int64_t n = a0.k1.n;
    for (int q = threadIdx.x; q < 9 * n_rec; q += MCX_BLOCK) lds[q] = 0.0;
    FastDateCvaLds* const dlds = (FastDateCvaLds*)(lds + ((9 * n_rec + 1) & ~1));      // (DK != 0) 16-byte aligned
    if constexpr (DK != 0) {
        // every date's record, its regression rows gathered from the coefficient table of this run
        const FastDateCva* __restrict__ dc = a0.cva_dates;
        const double* __restrict__ cf = a0.coeffs;
        const int n_dates = a0.n_dates;
        for (int q = threadIdx.x; q < 16 * n_dates; q += MCX_BLOCK) {
            const int t = q >> 4, e = q & 15;
            double v;
            if (e < FDC_HEAD) {
                v = ((const double*)(dc + t))[e];
            } else {
                const int off = e < FDC_HEAD + 3 ? dc[t].coeff_off0 : dc[t].coeff_off1;
                v = off >= 0 ? cf[off + (e - FDC_HEAD) % 3] : 0.0;
            }
            ((double*)dlds)[q] = v;
        }
    }
    // 1024-entry Box-Muller tables (32 KiB of LDS) where the sub-steps dominate and four blocks per CU still fit: the two-factor
    // rates / credit signature; 128 entries elsewhere (books with hundreds of per-date records need the LDS for those)
    constexpr int BMB = SIG == SIG_VAS_CIR_E ? 10 : 7;
    constexpr int BM = (INJECT || !SIMULATE) ? 0 : MCX_BM_LDS_DOUBLES_B(BMB);
    __shared__ double tab_lds[BM + MCX_EXP_LDS_DOUBLES];            // Box-Muller lookup tables | exp table
    const double* tab = nullptr;
    const double* etab = tab_lds + BM;
    mcx_exp_tab_load(tab_lds + BM);
    if (BM) { mcx_bm_load<BMB>(tab_lds); tab = tab_lds; }
    __syncthreads();
    const int64_t tiles = (n + TILE - 1) / TILE;
    double n_block = 0.0;

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const bool first_tile = tile == (int64_t)blockIdx.x;
        int64_t i[PPL];
        bool live[PPL];
        uint64_t path[PPL];
        double reg[PPL][NREG];                         // reg[q][2s], reg[q][2s+1] = state of slot s of the lane's q-th path
        double cfs[PPL], cva[PPL];
        int est[PPL];                                  // rights left of the book's (at most one) exercise product
        int n_init, n_steps;
        {
            KArgs& a = kargs_region(mcx_region_zero());          // tile prologue
            const auto& k = a.k1;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int64_t i_raw = tile * TILE + q * MCX_BLOCK + threadIdx.x;
                live[q] = i_raw < n;
                i[q] = live[q] ? i_raw : n - 1;        // dead lanes shadow the last path (no stores, no contribution)
                path[q] = k.path_offset + (uint64_t)i[q];
                sim_init_state<NSLOT, SIG>(k, reg[q]);
                cfs[q] = 0.0; cva[q] = 0.0;
                est[q] = a.init_state[0];
            }
            const int64_t rest = n - tile * TILE;
            n_block += (double)(rest < TILE ? rest : TILE);
            n_init = k.n_initial_store; n_steps = k.n_steps;
        }
        if (SIMULATE) {
        // ONE date call site: the dates that hold the initial state come first (their sub-step run is empty), then
        // alternately a run of sub-steps up to the next timeline date and that date's program
        int step = 0, t_init = 0;
#pragma unroll 1
        while (true) {
            const bool init = t_init < n_init;
            if (!init && step >= n_steps) break;
            int st = init ? t_init : -1;
            t_init += init ? 1 : 0;
            {
                const int zr0 = mcx_region_zero();      // arguments, Philox key schedule, Box-Muller coefficients of this run
                const auto& k = kargs_region(zr0).k1;
                const uint64_t seed = k.seed;
                const mcx_bm_coef bc = mcx_bm_coef_load(zr0);
                const mcx_bm_vconst vc = mcx_bm_vconst_make<BMB>(bc);  // constants kept in registers across the run of sub-steps
                // (DK = 1) the one high word of the launch's path indices, read where it is used like every other argument
                uint32_t path_hi = 0;
                CvaDrawConst dc = {};
                if constexpr (DK == 1) { path_hi = ((const MCX_KONST uint32_t*)&k.path_offset)[1]; dc = cva_draw_const_make(); }
#pragma unroll 1
                while (st < 0 && step < n_steps) {
                    if constexpr (SIG == SIG_GENERIC) {
                        // run-time model dispatch (every aux entry of every slot would have to be loaded ahead): path after path
#pragma unroll
                        for (int q = 0; q < PPL; ++q) sim_substep<NSLOT, NZ, INJECT, SIG, BMB, true>(k, step, path[q], i[q], reg[q], tab, seed, bc, &vc);   // POS: mcx_fused_create
                        st = ldk(&k.steps[step].store_idx);
                    } else {
                        // draws of all the lane's paths in ONE basic block (unguarded root, pair_from_words), one rare branch for the
                        // 2^-32 draws that may round to u = 1, then the state updates
                        double zz[PPL][NZ], uu[PPL];
                        bool rare = false;
                        // the scalar loads of this sub-step go out first: the draws below cover their latency
                        const StepData<NSLOT, NZ> sdat = sim_step_load<NSLOT, NZ, SIG>(k, step);
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (INJECT) {
#pragma unroll
                            for (int q = 0; q < PPL; ++q) sim_draw<NZ, true, SIG, BMB>(k, step, path[q], i[q], zz[q], uu[q], tab, seed, bc, &vc);
                        } else if constexpr (DK == 1) {
                            static_assert(NZ == 2, "one Philox block per path and sub-step");
                            uint32_t plo[PPL];
                            double za[PPL], zb[PPL];
#pragma unroll
                            for (int q = 0; q < PPL; ++q) plo[q] = (uint32_t)path[q];
                            rare = cva_draw_pairs<PPL, BMB>(seed, plo, path_hi, (uint32_t)step, 0u, za, zb, tab, bc, vc, dc);
#pragma unroll
                            for (int q = 0; q < PPL; ++q) { zz[q][0] = za[q]; zz[q][1] = zb[q]; uu[q] = 0.0; }
                        } else {
                            uint32_t st_q[PPL];
#pragma unroll
                            for (int q = 0; q < PPL; ++q) st_q[q] = (uint32_t)step;
                            rare = sim_draw_n<PPL, NZ, SIG, BMB>(k, st_q, path, zz, uu, tab, seed, bc, vc);
                        }
                        if (!INJECT && __builtin_expect(__any(rare), 0)) {
                            if constexpr (DK == 1) {
                                // only the low word of the path index is kept per lane
#pragma unroll
                                for (int q = 0; q < PPL; ++q)
                                    sim_draw<NZ, false, SIG, BMB, true>(k, step, ((uint64_t)path_hi << 32) | (uint32_t)path[q], i[q], zz[q], uu[q], tab, seed, bc, &vc);
                            } else {
#pragma unroll
                                for (int q = 0; q < PPL; ++q) sim_draw<NZ, false, SIG, BMB, true>(k, step, path[q], i[q], zz[q], uu[q], tab, seed, bc, &vc);
                            }
                        }
#pragma unroll
                        for (int q = 0; q < PPL; ++q) st = sim_apply_loaded<NSLOT, NZ, SIG, true>(k, sdat, reg[q], zz[q], uu[q]);   // POS: mcx_fused_create
                    }
                    ++step;
                }
            }
            if (st >= 0) {
                if constexpr (DK != 0) lean_date_cva<NSLOT, PPL>(dlds + st, reg, cva, etab);
                else lean_date<NSLOT, SIG, PPL, true>(st, i, live, first_tile, lds, reg, cfs, cva, est, etab);
            }
        }
        } else {
            auto load_row = [&](int t, double (&dst)[PPL][NREG]) {
                const auto& k = kargs_region(0).k1;
                const int D = k.n_state;
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int sl = 0; sl < NSLOT; ++sl) {
                        const bool bs = sig_kind(SIG, sl) >= 0 ? sig_is_bs(SIG, sl) : (k.slots[sl].kind == MCX_MODEL_BS);
                        const int c = k.slots[sl].state_off;
                        dst[q][2 * sl] = k.paths[((int64_t)t * D + c) * k.ld + i[q]];
                        dst[q][2 * sl + 1] = bs ? 0.0 : k.paths[((int64_t)t * D + c + 1) * k.ld + i[q]];
                    }
            };
            const int n_dates = kargs_region(0).n_dates;
            // the pass is a pure stream: two state buffers, the date loop unrolled by two so that each buffer is consumed where its
            // loads landed (a single call site with a rotating third buffer cost 32 register copies per path and date — a fifth of the
            // VALU work of the pass); the loads of date t+2 go out as soon as date t is done and have the program of date t+1 to land
            double bufb[PPL][NREG];
            load_row(0, reg);
            load_row(n_dates > 1 ? 1 : 0, bufb);
#pragma unroll 1
            for (int t = 0; t < n_dates; t += 2) {
                lean_date<NSLOT, SIG, PPL, false>(t, i, live, first_tile, lds, reg, cfs, cva, est, etab);
                if (t + 2 < n_dates) load_row(t + 2, reg);
                if (t + 1 < n_dates) {
                    lean_date<NSLOT, SIG, PPL, false>(t + 1, i, live, first_tile, lds, bufb, cfs, cva, est, etab);
                    if (t + 3 < n_dates) load_row(t + 3, bufb);
                }
            }
        }
        {
            KArgs& a = kargs_region(mcx_region_zero());          // tile epilogue: per-path quantities
#pragma unroll
            for (int q = 0; q < PPL; ++q) if (a.cfs && live[q]) a.cfs[i[q]] = cfs[q];
            if (a.rec_pv[0] >= 0) lean_record<PPL>(cfs, live, a.rec_pv[0], n_rec, first_tile, lds);
            if (a.rec_cva[0] >= 0) {
                const double lgd = a.lgd[0];
                double cc[PPL];
#pragma unroll
                for (int q = 0; q < PPL; ++q) cc[q] = cva[q] * lgd;
                lean_record<PPL>(cc, live, a.rec_cva[0], n_rec, first_tile, lds);
            }
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n_rec; r += MCX_BLOCK) {
        double s1 = 0.0, s2 = 0.0;
        for (int w = 0; w < 4; ++w) { s1 += lds[n_rec + (w * n_rec + r) * 2]; s2 += lds[n_rec + (w * n_rec + r) * 2 + 1]; }
        double* dst = a0.partials + ((int64_t)blockIdx.x * n_rec + r) * 4;
        dst[0] = n_block; dst[1] = lds[r]; dst[2] = s1; dst[3] = s2;
    }
}

// launch of one shape (paths per lane) of the kernel; returns the grid
template <int NSLOT, int NZ, int SIG, int PPL>
int launch_lean_shape(const FusedArgs& a, int full_steps, int n_cu, bool inject, bool simulate, hipStream_t s)
{
    const int64_t tiles = (a.k1.n + MCX_BLOCK * PPL - 1) / (MCX_BLOCK * PPL);
    const size_t lds = sizeof(double) * (size_t)((9 * a.n_rec + 1) & ~1);
    const size_t lds_cva = lds + sizeof(FastDateCvaLds) * (size_t)a.n_dates;
    // blocks that are really co-resident: __launch_bounds__(256, 4) guarantees the registers of 4 blocks per CU, but a book with
    // hundreds of records (one per metric date) adds dynamic LDS to the 34 KiB of tables and may leave room for 3 only; a grid
    // sized for 4 would then run its last quarter as a tail at a third of the occupancy
    auto residency = [&](auto kernel, size_t bytes) {
        thread_local std::map<std::pair<const void*, size_t>, int> cache;      // (the query costs microseconds: once per kernel and size)
        const auto key = std::make_pair((const void*)kernel, bytes);
        auto it = cache.find(key);
        if (it == cache.end()) {
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, MCX_BLOCK, bytes) != hipSuccess || per_cu < 1) per_cu = 1;
            it = cache.emplace(key, per_cu < MCX_LEAN_WAVES ? per_cu : MCX_LEAN_WAVES).first;
        }
        return (int64_t)it->second * n_cu;
    };
    auto sized = [&](int64_t resident) {
        if (tiles <= resident) return (int)tiles;
        const int64_t per = (tiles + resident - 1) / resident;  // equal number of tiles per block whenever the count divides
        return (int)((tiles + per - 1) / per);
    };
    int grid;
    if (!simulate) {
        auto kern = kf_lean<NSLOT, NZ, false, SIG, PPL, false>;
        grid = sized(residency(kern, lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(MCX_BLOCK), lds, s, a);
    } else if (inject) {
        auto kern = kf_lean<NSLOT, NZ, true, SIG, PPL, true>;
        grid = sized(residency(kern, lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(MCX_BLOCK), lds, s, a);
    } else {
        auto kern = kf_lean<NSLOT, NZ, false, SIG, PPL, true>;
        const int64_t resident = residency(kern, lds);
        if constexpr (SIG == SIG_VAS_CIR_E) {
            // the cva-date kernel, unless its date records in LDS (128 B per date) cost a block per CU or the launch's path
            // indices do not share one high word (the early Philox rounds of cva_draw_pairs take that word as a scalar).
            // A launch whose grid fills the chip (four blocks per CU, four waves per SIMD) draws through cva_draw_pairs, whose
            // scalar chain at the head of every sub-step and whose table reads the other waves of the SIMD cover: the backend sinks
            // stage C of those draws behind the rare-draw branch, away from the reads, and at four waves that order is the faster
            // one.  Any thinner grid (fewer tiles than resident blocks, or a tile count that sized() deals to fewer blocks) has
            // less to cover them with and keeps the staged draws of draw_pairs_staged (DK = 2).
            auto kern_cva = kf_lean<NSLOT, NZ, false, SIG, 2, true, 1>;         // (two paths per lane only: a full launch)
            auto kern_cva_thin = kf_lean<NSLOT, NZ, false, SIG, PPL, true, 2>;
            const bool one_high_word = ((a.k1.path_offset + (uint64_t)(a.k1.n - 1)) >> 32) == (a.k1.path_offset >> 32);
            if (a.cva_dates && one_high_word) {
                grid = sized(resident);
                if (PPL == 2 && grid >= resident) {
                    if (residency(kern_cva, lds_cva) >= resident) {
                        hipLaunchKernelGGL(kern_cva, dim3(grid), dim3(MCX_BLOCK), lds_cva, s, a);
                        return grid;
                    }
                } else if (residency(kern_cva_thin, lds_cva) >= resident) {
                    hipLaunchKernelGGL(kern_cva_thin, dim3(grid), dim3(MCX_BLOCK), lds_cva, s, a);
                    return grid;
                }
            }
        }
        grid = sized(resident);
        // a pass prepared for the cva-date kernel stops after the last date that adds to the CVA (fused_run_impl); every other
        // kernel runs the whole step table
        FusedArgs g = a;
        g.k1.n_steps = full_steps;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(MCX_BLOCK), lds, s, g);
    }
    return grid;
}

template <int NSLOT, int NZ, int SIG>
void launch_lean(const FusedArgs& a, int full_steps, int n_cu, bool inject, bool simulate, hipStream_t s, int* grid_out)
{
    // Full shape: two paths per lane where both fit the 128-VGPR budget of 4 waves per SIMD (the generic run-time-dispatch kernels
    // of several sub-models carry every model's step code and would spill: one path per lane).  512 paths per block-tile, 4 blocks
    // per CU: 2^19 paths fill the chip once.
    constexpr int PPL = (SIG == SIG_GENERIC && NSLOT >= 2) ? 1 : 2;
#ifdef MCX_LEAN_AB
    // tools/build_variants.sh only (never defined in the product build): the shape picked by the environment, 10 * PPL + 1
    if (simulate && !inject) {
        const char* sh = getenv("MCX_LEAN_SHAPE");
        const int code = sh ? atoi(sh) : 0;
        if (code == 11) { *grid_out = launch_lean_shape<NSLOT, NZ, SIG, 1>(a, full_steps, n_cu, inject, simulate, s); return; }
        if (code == 21) { *grid_out = launch_lean_shape<NSLOT, NZ, SIG, 2>(a, full_steps, n_cu, inject, simulate, s); return; }
    }
#endif
    // Small path counts (one GPU's share of a strong-scaled run: 2^20 paths over 8 GPUs = 2^17 each): the full shape would put one
    // wave on a SIMD.  A wave of this kernel spends a third of its cycles on wave-uniform work — scalar loads of the step and date
    // records and their waits, SALU control (SQ counters, profiles/README.md) — which a second wave on the SIMD overlaps with its
    // own VALU work and a single wave cannot: below half a chip-filling launch one path per lane (twice the waves) is faster,
    // 0.176 against 0.195 ms at 131,072 paths, equal at 262,144, slower from there on (the scalar work per path doubles).
    const int64_t full_tiles = (a.k1.n + MCX_BLOCK * PPL - 1) / (MCX_BLOCK * PPL);
    if (PPL == 2 && simulate && !inject && full_tiles < (int64_t)2 * n_cu) {
        *grid_out = launch_lean_shape<NSLOT, NZ, SIG, 1>(a, full_steps, n_cu, inject, simulate, s);
        return;
    }
    *grid_out = launch_lean_shape<NSLOT, NZ, SIG, PPL>(a, full_steps, n_cu, inject, simulate, s);
}

}  // namespace

// host entry used by kf_fused.hip (fused_run_impl); returns the grid size (number of per-block partial records), or -1 when
// the (slots, z) shape has no instantiation
int mcx_launch_kf_lean(const FusedArgs& a, const mcx_sim_desc& sd, int n_cu, bool inject, bool simulate, hipStream_t s)
{
    int grid = -1;
#ifdef MCX_LEAN_ONE_SIG
    // tools/asm_mix.py only (never defined in the product build): the one signature it measures, nothing else instantiated
    if (mcx_sim_signature(sd) == SIG_VAS_CIR_E) launch_lean<2, 2, SIG_VAS_CIR_E>(a, sd.n_steps, n_cu, inject, simulate, s, &grid);
#else
    mcx_dispatch_signature<4>(sd, [&](auto nslot, auto nz, auto sig) {
        launch_lean<decltype(nslot)::value, decltype(nz)::value, decltype(sig)::value>(a, sd.n_steps, n_cu, inject, simulate, s, &grid);
    });
#endif
    return grid;
}
