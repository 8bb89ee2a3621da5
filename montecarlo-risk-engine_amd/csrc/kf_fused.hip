// kf_fused.hip — the fused main-simulation pass: K1 (Philox + Box-Muller + Cholesky + SDE step) + K2 (requests,
// cashflows, exposures) + K4 (PV / EPE / ENE / CVA reductions) in ONE launch, no intermediate tensor in HBM.
//
// Reference dataflow replaced (controller/controller.py:677-694): generate_paths -> paths[N,T,D] (1.6 GB at config 3)
// -> resolve_requests (~2.4 GB) -> evaluate_products -> exposures[E,N] (0.4 GB) -> metric reductions.  Here a lane keeps
// its path's state in VGPRs, runs the book's events of a timeline date right after the sub-steps that reach it (every
// atom of such an event reads the state of THAT date), and folds the result into per-path accumulators (cashflows, CVA
// integrand) and per-date block accumulators (EPE / ENE) that live in LDS across the block's path tiles.
//
// Block-level reduction design: per record r the block keeps a shift c_r (value of the first path it sees) and, per wave,
// the pair (sum (x-c), sum (x-c)^2) in LDS; every date costs one wave64 shuffle reduction per record.  Blocks write one
// (n, c, s1, s2) record each; a tiny second kernel merges blocks with Chan's update (deterministic, no float atomics).
#include "kf_common.h"

#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdlib>

namespace {

// The book's events + metric operations of ONE timeline date for one lane.  The date's program chunk sits in the wave's
// private LDS slot (`chunk`): all 64 lanes read the same addresses (LDS broadcast, no bank conflicts), so walking the
// program costs ds_read latency (~64-128 clk) instead of a chain of dependent L2 round trips per record.
template <int NSLOT, int SIG, int NNS, int NSTA, bool STORE>
__device__ __forceinline__ void kf_on_date(KArgs& a, int t, int64_t i, bool live, bool first_tile, double* __restrict__ lds,
                                           const unsigned char* __restrict__ chunk, const double (&reg)[2 * NSLOT],
                                           double (&cfs)[NNS], double (&cva)[NNS], int (&est)[NSTA])
{
    constexpr int NREG = 2 * NSLOT;
    const auto& k = a.k1;
    const int n_rec = a.n_rec;
    if (STORE && k.paths && live) sim_store_state<NSLOT, SIG>(k, t, i, reg);
    const ChunkHeader* hdp = (const ChunkHeader*)chunk;
    ChunkHeader hd;
    hd.n_ev = RFL(hdp->n_ev); hd.n_mop = RFL(hdp->n_mop); hd.n_terms = RFL(hdp->n_terms); hd.bytes = 0;
    const FEvent* __restrict__ evs = (const FEvent*)(chunk + sizeof(ChunkHeader));
    const FTerm* __restrict__ terms = (const FTerm*)(evs + hd.n_ev);
    const FMetricOp* __restrict__ mops = (const FMetricOp*)(terms + hd.n_terms);
    double e_ns[NNS];
#pragma unroll
    for (int q = 0; q < NNS; ++q) e_ns[q] = 0.0;
    double inv_num = 0.0;
#pragma unroll 1
    for (int q = 0; q < hd.n_ev; ++q) {
        const FEvent& ev = evs[q];
        struct { int kind, flags, term_begin, term_end, coeff_off, ns, sidx, init_state; double strike, sign; const FAtom &num, &x; } e =
            {RFL(ev.kind), RFL(ev.flags), RFL(ev.term_begin), RFL(ev.term_end), RFL(ev.coeff_off), RFL(ev.ns), RFL(ev.sidx),
             RFL(ev.init_state), ev.strike, ev.sign, ev.num, ev.x};
        if (!(e.flags & FE_SAME_NUM)) inv_num = 1.0 / f_atom<NREG>(e.num, reg);
        double v = 0.0;
        if (e.kind <= MCX_EV_EXERCISE) {
            double val = 0.0, glog = 0.0;
            const int basket = e.kind == MCX_EV_OPTION ? RFL((int)ev.aux[0]) : 0;      // basket aggregation mode (basket_option.py)
#pragma unroll 1
            for (int j = e.term_begin; j < e.term_end; ++j) {
                const double av = f_atom<NREG>(terms[j].atom, reg);
                val = fma(terms[j].w, av, val);
                if (basket == 1 || basket == 2) glog = fma(terms[j].w, mcx_log(av + 1e-10), glog);
            }
            if (e.kind == MCX_EV_CASHFLOW) {
                v = val * inv_num;
            } else {
                const double imm = fmax(e.sign * (val - e.strike), 0.0);
                if (e.kind == MCX_EV_OPTION) {
                    v = imm * inv_num;
                    if (basket == 3) {                                   // binary payoff: fuzzy indicator (binary_option.py:38-43)
                        const double dot = fmin(fmax((val - e.strike + ev.aux[2]) / (2.0 * ev.aux[2]), 0.0), 1.0);
                        v = ev.aux[1] * (e.sign > 0.0 ? dot : 1.0 - dot) * inv_num;
                    } else if (basket) {
                        const double geo = fmax(e.sign * (mcx_exp(glog) - e.strike), 0.0);
                        v = (basket == 1 ? geo : imm - geo + ev.aux[1]) * inv_num;
                    }
                } else {
                    int s = 0;
#pragma unroll
                    for (int w = 0; w < NSTA; ++w) s = (e.sidx == w) ? est[w] : s;
                    double cont = 0.0, cont_ex = 0.0;
                    if (e.coeff_off >= 0) {
                        const double x = f_atom<NREG>(e.x, reg);
                        cont = f_poly(a.coeffs + e.coeff_off + s * a.n_basis, a.n_basis, x);
                        if (RFL((int)ev.aux[0]) == 1)            // FlexiCall: continuation after exercising (flexicall.py:118-133)
                            cont_ex = s > 0 ? f_poly(a.coeffs + e.coeff_off + (s - 1) * a.n_basis, a.n_basis, x) : 0.0;
                    }
                    const bool ex = (imm + cont_ex > cont) && (s > 0);
                    v = ex ? imm * inv_num : 0.0;
#pragma unroll
                    for (int w = 0; w < NSTA; ++w) est[w] = (e.sidx == w && ex) ? s - 1 : est[w];
                }
            }
#pragma unroll
            for (int w = 0; w < NNS; ++w) cfs[w] += (NNS == 1 || e.ns == w) ? v : 0.0;
        } else {
            if (e.kind == MCX_EV_EXPO_POLY) {
                int s = e.init_state;
#pragma unroll
                for (int w = 0; w < NSTA; ++w) s = (e.sidx == w) ? est[w] : s;
                const double x = f_atom<NREG>(e.x, reg);
                if (e.coeff_off >= 0)
                    v = (e.sidx < 0 ? f_poly_uniform(a.coeffs, e.coeff_off + e.init_state * a.n_basis, a.n_basis, x)
                                    : f_poly(a.coeffs + e.coeff_off + s * a.n_basis, a.n_basis, x)) * inv_num;
            }
#pragma unroll
            for (int w = 0; w < NNS; ++w) e_ns[w] += (NNS == 1 || e.ns == w) ? v : 0.0;
        }
    }
    const int row = ldk(a.date_row + t);
    if (a.expo && row >= 0 && live) {
        for (int w = 0; w < a.n_ns; ++w) {
            double ev = e_ns[0];
#pragma unroll
            for (int q = 1; q < NNS; ++q) ev = (w == q) ? e_ns[q] : ev;
            a.expo[((int64_t)w * a.n_expo_rows + row) * a.ld_out + i] = ev;
        }
    }
#pragma unroll 1
    for (int q = 0; q < hd.n_mop; ++q) {
        const FMetricOp& mv = mops[q];
        struct { int ns, rec_profile, has_cva; double threshold; const FAtom &surv, &cond; } mo =
            {RFL(mv.ns), RFL(mv.rec_profile), RFL(mv.has_cva), mv.threshold, mv.surv, mv.cond};
        double e = e_ns[0];
#pragma unroll
        for (int w = 1; w < NNS; ++w) e = (mo.ns == w) ? e_ns[w] : e;
        const double u = dev_thr(e, mo.threshold);
        if (mo.rec_profile >= 0) {
            lean_record<1>({fmax(u, 0.0)}, {live}, mo.rec_profile, n_rec, first_tile, lds);
            lean_record<1>({fmin(u, 0.0)}, {live}, mo.rec_profile + 1, n_rec, first_tile, lds);
        }
        if (mo.has_cva) {
            const double sp = f_atom<NREG>(mo.surv, reg);
            const double cs = f_atom<NREG>(mo.cond, reg);
            const double inc = fmax(u, 0.0) * (sp * (1.0 - cs));
#pragma unroll
            for (int w = 0; w < NNS; ++w) cva[w] += (NNS == 1 || mo.ns == w) ? inc : 0.0;
        }
    }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// NNS = compile-time bound on netting sets (1 or MCX_FUSED_MAX_NS), NST = bound on exercise products (0 -> none).
// NPF = 1 KiB pieces of the NEXT date's program chunk each wave prefetches into VGPRs (one coalesced global_load_dwordx4
// per piece, issued before the sub-steps that lead to that date, written to the wave's LDS slot just before use: the HBM/L2
// latency hides under ~5 sub-steps of RNG + SDE work).  NPF = 0: chunks larger than 2 KiB are copied at use, or no date is
// interpreted.
// SIMULATE = false: the same event/metric program runs on a paths tensor produced earlier by K1 (`k.paths` is then the
// INPUT [date][state][path]): one pass over the paths replaces K2 + K4 and writes no exposure matrix unless asked to.
// The arguments are read per code region (block prologue, tile prologue, one run of sub-steps, one date, per-path epilogue,
// block epilogue) through kargs_region, as in kf_lean.hip: no argument SGPR is kept alive across the loops.
template <int NSLOT, int NZ, bool INJECT, int SIG, int NNS, int NST, int NPF, bool SIMULATE>
__global__ __launch_bounds__(MCX_BLOCK) void kf_fused(const FusedArgs)      // read through kargs_region(), never by name
{
    constexpr int NREG = 2 * NSLOT;
    constexpr int NSTA = NST > 0 ? NST : 1;
    constexpr int NPFA = NPF > 0 ? NPF : 1;
    extern __shared__ double lds[];
    KArgs& a0 = kargs_region(0);                                     // block prologue and epilogue
    const int n_rec = a0.n_rec;
    const int64_t n = a0.k1.n;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int rec_area = (9 * n_rec + 1) & ~1;                       // doubles; keeps the program slots 16-byte aligned
    unsigned char* slot = (unsigned char*)(lds + rec_area) + (size_t)wv * a0.chunk_cap;      // wave-private program slot
    for (int q = threadIdx.x; q < 9 * n_rec; q += MCX_BLOCK) lds[q] = 0.0;
    constexpr int BM = (SIMULATE && !INJECT) ? MCX_BM_LDS_DOUBLES : 0;
    constexpr int NE = NNS == 1 ? MCX_EXP_LDS_DOUBLES : 0;          // lean_date runs the straight-line dates of one netting set
    __shared__ double tab_lds[BM + NE > 0 ? BM + NE : 1];           // Box-Muller lookup tables | exp table
    const double* tab = BM ? tab_lds : nullptr;
    const double* etab = tab_lds + BM;
    if (BM) mcx_bm_load(tab_lds);
    if (NE) mcx_exp_tab_load(tab_lds + BM);
    __syncthreads();
    const int64_t tiles = (n + MCX_BLOCK - 1) / MCX_BLOCK;
    double n_block = 0.0;

    u32x4 pf[NPFA];
    auto prefetch = [&](KArgs& a, int t) {   // issue the loads of date t's chunk (NPF > 0)
        if (NPF > 0 && t < a.n_dates) {
            const int off = ldk(a.date_off + t), end = ldk(a.date_off + t + 1);
#pragma unroll
            for (int p = 0; p < NPFA; ++p) {
                const int b = off + (p * 64 + lane) * 16;
                pf[p] = b < end ? *(const u32x4*)(a.prog + b) : u32x4{0, 0, 0, 0};
            }
        }
    };
    auto stage = [&](KArgs& a, int t) {      // make date t's chunk visible in the wave's LDS slot
        if (NPF > 0) {
#pragma unroll
            for (int p = 0; p < NPFA; ++p) ((u32x4*)slot)[p * 64 + lane] = pf[p];
        } else {
            const int off = ldk(a.date_off + t), end = ldk(a.date_off + t + 1);
            for (int b = lane * 16; b < end - off; b += 64 * 16) *(u32x4*)(slot + b) = *(const u32x4*)(a.prog + off + b);
        }
    };

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const bool first_tile = tile == (int64_t)blockIdx.x;
        const int64_t i_raw = tile * MCX_BLOCK + threadIdx.x;
        const bool live = i_raw < n;
        const int64_t i = live ? i_raw : n - 1;            // dead lanes shadow the last path (no stores, no contribution)
        { const int64_t rest = n - tile * MCX_BLOCK; n_block += (double)(rest < MCX_BLOCK ? rest : MCX_BLOCK); }

        double reg1[1][NREG];                              // the one-path shape of lean_date
        double (&reg)[NREG] = reg1[0];                     // reg[2s], reg[2s+1] = state of slot s
        double cfs[NNS], cva[NNS];
        int est[NSTA];
        uint64_t path;
        int n_dates, n_init, n_steps;
        {
            KArgs& a = kargs_region(mcx_region_zero());   // tile prologue
            sim_init_state<NSLOT, SIG>(a.k1, reg);
#pragma unroll
            for (int q = 0; q < NNS; ++q) { cfs[q] = 0.0; cva[q] = 0.0; }
#pragma unroll
            for (int q = 0; q < NSTA; ++q) est[q] = a.init_state[q];
            path = a.k1.path_offset + (uint64_t)i;
            n_dates = a.n_dates; n_init = a.k1.n_initial_store; n_steps = a.k1.n_steps;
            prefetch(a, 0);
        }

        auto on_date = [&](int t, auto store) {
            constexpr bool ST = decltype(store)::value;
            KArgs& a = kargs_region(mcx_region_zero());   // one date
            if constexpr (NNS == 1) {
                if (ldk(&a.fast[t].valid) != 0) {          // a straight-line record: the date program of kf_lean.hip
                    // such a date has no chunk: the prefetched pieces are dead (kept live through lean_date, they cost 8 VGPRs)
#pragma unroll
                    for (int p = 0; p < NPFA; ++p) pf[p] = u32x4{0, 0, 0, 0};
                    int est1[1] = {est[0]};                // (mcx_fused_create: a stateful event of such a date has sidx 0)
                    lean_date<NSLOT, SIG, 1, ST>(t, {i}, {live}, first_tile, lds, reg1, cfs, cva, est1, etab);
                    est[0] = est1[0];
                    prefetch(a, t + 1);
                    return;
                }
            }
            stage(a, t);
            prefetch(a, t + 1);
            kf_on_date<NSLOT, SIG, NNS, NSTA, ST>(a, t, i, live, first_tile, lds, slot, reg, cfs, cva, est);
        };
        // timeline dates are visited in increasing order, each once
        if (SIMULATE) {
            for (int t = 0; t < n_init; ++t) on_date(t, std::integral_constant<bool, true>());
            // two nested loops: the inner one is the bare sub-step recursion up to the next timeline date (register
            // allocation then treats it as the hot loop: the date program's scalars are not kept alive / spilled through it)
            int step = 0;
#pragma unroll 1
            while (step < n_steps) {
                int st;
                {
                    const int zr = mcx_region_zero();     // one run of sub-steps: arguments, Box-Muller coefficients
                    const auto& k = kargs_region(zr).k1;
                    const mcx_bm_coef bc = mcx_bm_coef_load(zr);
#pragma unroll 1
                    do {
                        sim_substep<NSLOT, NZ, INJECT, SIG>(k, step, path, i, reg, tab, k.seed, bc);
                        st = ldk(&k.steps[step].store_idx);
                        ++step;
                    } while (st < 0 && step < n_steps);
                }
                if (st >= 0) on_date(st, std::integral_constant<bool, true>());
            }
        } else {
            double nxt[NREG];
            auto load_row = [&](int t, double (&dst)[NREG]) {
                const auto& k = kargs_region(mcx_region_zero()).k1;
                const int D = k.n_state;
#pragma unroll
                for (int s = 0; s < NSLOT; ++s) {
                    const bool bs = sig_kind(SIG, s) >= 0 ? sig_is_bs(SIG, s) : (k.slots[s].kind == MCX_MODEL_BS);
                    const int c = k.slots[s].state_off;
                    dst[2 * s] = k.paths[((int64_t)t * D + c) * k.ld + i];
                    dst[2 * s + 1] = bs ? 0.0 : k.paths[((int64_t)t * D + c + 1) * k.ld + i];
                }
            };
            load_row(0, nxt);
#pragma unroll 1
            for (int t = 0; t < n_dates; ++t) {
#pragma unroll
                for (int q = 0; q < NREG; ++q) reg[q] = nxt[q];
                if (t + 1 < n_dates) load_row(t + 1, nxt);      // next date's state streams in while this date's ops run
                on_date(t, std::integral_constant<bool, false>());
            }
        }
        {
            KArgs& a = kargs_region(mcx_region_zero());   // per-path epilogue
            for (int w = 0; w < a.n_ns; ++w) {
                double cv = cfs[0], cc = cva[0];
#pragma unroll
                for (int q = 1; q < NNS; ++q) { cv = (w == q) ? cfs[q] : cv; cc = (w == q) ? cva[q] : cc; }
                if (a.cfs && live) a.cfs[(int64_t)w * a.ld_out + i] = cv;
                if (a.rec_pv[w] >= 0) lean_record<1>({cv}, {live}, a.rec_pv[w], n_rec, first_tile, lds);
                if (a.rec_cva[w] >= 0) lean_record<1>({cc * a.lgd[w]}, {live}, a.rec_cva[w], n_rec, first_tile, lds);
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

// merge per-block records (Chan, Golub, LeVeque pairwise update) -> out[r] = (n, mean, 0, M2).
// One 256-thread block per record: every thread folds a strided subset of the block records (independent loads in
// flight), the 256 partial triples are then combined through LDS.  (A one-thread serial merge over 2048 dependent loads
// took 0.8 ms — a quarter of the whole pass.)
__global__ __launch_bounds__(MCX_BLOCK) void kf_merge(const double* __restrict__ partials, int n_rec, int n_blocks, mcx_acc* __restrict__ out)
{
    const int r = blockIdx.x;
    __shared__ double sN[MCX_BLOCK], sM[MCX_BLOCK], sQ[MCX_BLOCK];
    double N = 0.0, mean = 0.0, M2 = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += MCX_BLOCK) {
        const double* p = partials + ((int64_t)b * n_rec + r) * 4;
        const double n = p[0];
        if (n > 0.0) chan_merge(N, mean, M2, n, p[1] + p[2] / n, fmax(p[3] - p[2] * p[2] / n, 0.0));
    }
    sN[threadIdx.x] = N; sM[threadIdx.x] = mean; sQ[threadIdx.x] = M2;
    __syncthreads();
    for (int stride = MCX_BLOCK / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) {
            double a = sN[threadIdx.x], b = sM[threadIdx.x], c = sQ[threadIdx.x];
            chan_merge(a, b, c, sN[threadIdx.x + stride], sM[threadIdx.x + stride], sQ[threadIdx.x + stride]);
            sN[threadIdx.x] = a; sM[threadIdx.x] = b; sQ[threadIdx.x] = c;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[r].n = sN[0]; out[r].shift = sM[0]; out[r].s1 = 0.0; out[r].s2 = sQ[0]; }
}

// The kernel a pass launches, chosen by kf_route() below: kf_lean (every date straight-line), or kf_fused with these template
// bounds.  launch_kf maps the fields one to one onto instantiations; mcx_fused_describe reports the same record.
struct KfRoute {
    int kernel;                // MCX_ROUTE_NONE / MCX_ROUTE_LEAN / MCX_ROUTE_FUSED
    bool inject;
    int nns, nst, npf;         // kf_fused's NNS, NST and NPF (0 unless kernel == MCX_ROUTE_FUSED)
};

template <int NSLOT, int NZ, int SIG>
void launch_kf(const FusedArgs& a, int grid, size_t lds, const KfRoute& r, bool simulate, hipStream_t s)
{
    const int npf = r.npf;
#define MCX_KF(INJ, NNS, NST, NPF) do { if (simulate) hipLaunchKernelGGL((kf_fused<NSLOT, NZ, INJ, SIG, NNS, NST, NPF, true>), dim3(grid), dim3(MCX_BLOCK), lds, s, a); \
        else if (!INJ) hipLaunchKernelGGL((kf_fused<NSLOT, NZ, false, SIG, NNS, NST, NPF, false>), dim3(grid), dim3(MCX_BLOCK), lds, s, a); } while (0)
#define MCX_KF_NPF(INJ, NNS, NST) do { if (npf == 1) MCX_KF(INJ, NNS, NST, 1); else if (npf == 2) MCX_KF(INJ, NNS, NST, 2); else MCX_KF(INJ, NNS, NST, 0); } while (0)
    if (r.inject) {
        if (r.nns == 1 && r.nst == 0) MCX_KF_NPF(true, 1, 0);
        else if (r.nns == 1) MCX_KF(true, 1, MCX_FUSED_MAX_STATEFUL, 0);
        else MCX_KF(true, MCX_FUSED_MAX_NS, MCX_FUSED_MAX_STATEFUL, 0);
    } else {
        if (r.nns == 1 && r.nst == 0) MCX_KF_NPF(false, 1, 0);
        else if (r.nns == 1) MCX_KF_NPF(false, 1, MCX_FUSED_MAX_STATEFUL);
        else MCX_KF(false, MCX_FUSED_MAX_NS, MCX_FUSED_MAX_STATEFUL, 0);
    }
#undef MCX_KF_NPF
#undef MCX_KF
}

}  // namespace

struct mcx_fused {
    const mcx_sim* sim = nullptr;
    const mcx_book* book = nullptr;
    int n_rec = 0, n_ns = 0, n_dates = 0, n_expo_rows = 0, n_stateful = 0, want_pv = 0;
    unsigned char* d_prog = nullptr;
    FastDate* d_fast = nullptr;
    int32_t* d_date_off = nullptr;
    int32_t* d_date_row = nullptr;
    int chunk_cap = 0, npf = 0, max_chunk = 0;      // max_chunk: bytes of the largest interpreted chunk (0: none)
    int lean = 0;              // every date has a FastDate record kf_lean.hip can run (valid != 0)
    FastDateCva* d_cva = nullptr;      // [n_dates] when every date runs in the cva-date kernel of kf_lean.hip, else nullptr
    int cva_steps = 0;         // (d_cva) sub-steps up to and including the last one that stores a date with a CVA increment
    LeanTerm* d_lterms = nullptr;
    double* d_vcoef = nullptr; // this object's copy of the exercise-value polynomial coefficients (the book may rebuild its own)
    int32_t rec_pv[MCX_FUSED_MAX_NS] = {}, rec_cva[MCX_FUSED_MAX_NS] = {};
    double lgd[MCX_FUSED_MAX_NS] = {};
    int32_t init_state[MCX_FUSED_MAX_STATEFUL] = {};
    std::vector<int32_t> date_desc;    // [n_dates][2] host copy of every FastDate's (valid, flags): what mcx_fused_describe reports
    double* d_partials = nullptr;
    size_t partial_bytes = 0;
    mcx_acc* d_out = nullptr;
    // optional timing of the main kernel alone (mcx_fused_set_timing): event pairs around its launch, on the launch stream
    mutable hipEvent_t tev[2 * MCX_FUSED_TIMING_RING] = {};
    mutable int timing = 0, t_count = 0, t_launch = 0;      // timing: 0 off, k > 0: every k-th launch is timed
};

static void fused_timing_off(mcx_fused* f)
{
    if (f->timing) for (int q = 0; q < 2 * MCX_FUSED_TIMING_RING; ++q) hipEventDestroy(f->tev[q]);
    f->timing = 0; f->t_count = 0; f->t_launch = 0;
}

extern "C" int mcx_fused_set_timing(mcx_fused* f, int32_t enable)
{
    if (!f) return -1;
    fused_timing_off(f);
    if (enable) {
        for (int q = 0; q < 2 * MCX_FUSED_TIMING_RING; ++q)
            if (hipEventCreate(&f->tev[q]) != hipSuccess) { for (int r = 0; r < q; ++r) hipEventDestroy(f->tev[r]); return -100; }
        f->timing = enable > 0 ? enable : 1;
    }
    return 0;
}

extern "C" int mcx_fused_kernel_times(mcx_fused* f, float* h_ms, int32_t capacity, int32_t* n_out)
{
    if (!f || !h_ms || !n_out) return -1;
    *n_out = 0;
    if (!f->timing) return 0;
    const int n = f->t_count < capacity ? f->t_count : capacity;
    for (int q = 0; q < n; ++q) {
        if (hipEventSynchronize(f->tev[2 * q + 1]) != hipSuccess) return -100;
        if (hipEventElapsedTime(&h_ms[q], f->tev[2 * q], f->tev[2 * q + 1]) != hipSuccess) return -100;
    }
    *n_out = n;
    f->t_count = 0; f->t_launch = 0;
    return 0;
}

extern "C" void mcx_fused_destroy(mcx_fused* f)
{
    if (!f) return;
    fused_timing_off(f);
    hipFree(f->d_lterms); hipFree(f->d_vcoef); hipFree(f->d_cva); hipFree(f->d_prog); hipFree(f->d_fast); hipFree(f->d_date_off); hipFree(f->d_date_row); hipFree(f->d_partials); hipFree(f->d_out);
    delete f;
}

extern "C" int mcx_fused_num_records(const mcx_fused* f) { return f ? f->n_rec : -1; }

// ---- mcx_fused_create: the plan of a pass, built on the host stage by stage (no stage calls HIP), then uploaded -----------------
namespace {

// What the stages decide: the tables the kernels read, exactly as uploaded, and the scalars of the launch.
struct FusedPlan {
    std::vector<unsigned char> prog;       // chunks of the interpreted dates (header | events | terms | metric ops), 16-byte aligned
    std::vector<FastDate> fast;            // [n_dates] (a date that is not straight-line keeps what was derived before it failed)
    std::vector<FastDateCva> cva_dates;    // [n_dates], uploaded when cva_only
    std::vector<LeanTerm> lterms;          // exponential terms of the exercise values + one spare entry
    std::vector<double> vcoef;             // value-polynomial coefficients + one spare block
    std::vector<int32_t> date_off, date_row;
    int n_rec = 0, n_stateful = 0, npf = 0, chunk_cap = 0, max_chunk = 0, cva_steps = 0;
    bool lean = false, cva_only = false;
    int32_t rec_pv[MCX_FUSED_MAX_NS], rec_cva[MCX_FUSED_MAX_NS];
    double lgd[MCX_FUSED_MAX_NS];
    int32_t init_state[MCX_FUSED_MAX_STATEFUL] = {};
};

// the book's program per timeline date before it is packed or turned into FastDate records (product order preserved)
struct DateLists {
    std::vector<std::vector<FEvent>> events;
    std::vector<std::vector<int>> event_q;          // book index of each bucketed event
    std::vector<std::vector<FTerm>> terms;
    std::vector<std::vector<FMetricOp>> mops;
    explicit DateLists(int T) : events(T), event_q(T), terms(T), mops(T) {}
};

// why the book is not fusable: the reason recorded last is the one reported (the stages stop at the end of the event or metric
// operation that recorded it)
struct Refusal {
    bool ok = true;
    std::string why;
    void operator()(const char* reason) { ok = false; why = reason; }
};

// stage 1: the arguments, in the order their failures are reported
int check_arguments(mcx_handle* h, const mcx_sim_desc& sd, const mcx_book* book, const mcx_fused_desc* d)
{
    if (book->n_state != sd.n_state) MCX_FAIL(h, -2, "mcx_fused_create: book and sim disagree on the state dimension");
    if (d->n_netting_sets < 1 || d->n_netting_sets > MCX_FUSED_MAX_NS || d->n_netting_sets != book->n_netting_sets)
        MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: %d netting sets (max %d)", book->n_netting_sets, MCX_FUSED_MAX_NS);
    if (d->n_expo_rows != book->n_expo_rows) MCX_FAIL(h, -2, "mcx_fused_create: n_expo_rows mismatch");
    for (int s = 0; s < sd.n_slots; ++s)
        if (sd.slots[s].kind == MCX_MODEL_S2F) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: the Schwartz two-factor spot is a derived state column");
    if ((int)book->h_event_t_idx.size() != book->n_events) MCX_FAIL(h, -2, "mcx_fused_create: internal (event dates missing)");
    return 0;
}

// state column -> lane register
void state_registers(const mcx_sim_desc& sd, int (&col_reg)[MCX_MAX_STATE])
{
    for (int s = 0; s < sd.n_slots; ++s) {
        col_reg[sd.slots[s].state_off] = 2 * s;
        if (sd.slots[s].kind != MCX_MODEL_BS) col_reg[sd.slots[s].state_off + 1] = 2 * s + 1;
    }
}

FAtom fatom(const mcx_atom& q, int t_event, const int* col_reg, Refusal& no)
{
    FAtom o; o.a = q.a; o.d = q.d; o.b = q.b; o.c0 = q.c0; o.c1 = q.c1; o.reg = -1;
    o.parts = (q.b != 0.0 ? FA_EXP : 0) | ((q.a != 0.0 || q.d != 0.0) ? FA_AFFINE : 0);
    if (q.col >= 0) {
        if (q.t_idx != t_event) no("an event reads the state of another date (unequal swap tenors)");
        o.reg = col_reg[q.col];
    }
    return o;
}
FAtom fatom(const DevAtom& q, int t_event, const int* col_reg, Refusal& no)
{
    mcx_atom o; o.t_idx = q.t_idx; o.col = q.col; o.a = q.a; o.d = q.d; o.b = q.b; o.c0 = q.c0; o.c1 = q.c1;
    return fatom(o, t_event, col_reg, no);
}

// stage 2: the book's events and their terms bucketed by timeline date; the slots and initial states of the exercise products
void bucket_events(const mcx_book& book, int T, const int* col_reg, FusedPlan& p, DateLists& dl, Refusal& no)
{
    const DevEventVec& hev = book.h_events;
    const std::vector<DevTerm>& hte = book.h_terms;
    for (int pi = 0; pi < book.n_products && no.ok; ++pi) {
        const DevProduct& pr = book.h_products[pi];
        if (pr.ev_end == pr.ev_begin) continue;
        int sidx = -1;
        if (pr.n_states > 1) {
            if (p.n_stateful >= MCX_FUSED_MAX_STATEFUL) { no("too many exercise products"); break; }
            sidx = p.n_stateful;
            p.init_state[p.n_stateful++] = pr.init_state;
        }
        for (int q = pr.ev_begin; q < pr.ev_end && no.ok; ++q) {
            const DevEvent& e = hev[q];
            const int t = book.h_event_t_idx[q];
            if (t < 0 || t >= T) { no("event date out of range"); break; }
            FEvent fe;
            memset(&fe, 0, sizeof(fe));
            fe.kind = e.kind; fe.flags = e.flags; fe.coeff_off = e.coeff_off; fe.row = e.row; fe.ns = pr.netting_set; fe.sidx = sidx;
            fe.init_state = pr.init_state; fe.n_states = pr.n_states; fe.strike = e.strike; fe.sign = e.sign;
            for (int w = 0; w < 4; ++w) fe.aux[w] = e.aux[w];
            if (e.kind == MCX_EV_OPTION && (e.aux[0] == 4.0 || e.aux[0] == 5.0)) no("barrier monitoring is evaluated by the book kernel (K2)");
            fe.num = fatom(e.num, t, col_reg, no);
            fe.x = fatom(e.x, t, col_reg, no);
            std::vector<FTerm>& terms = dl.terms[t];
            fe.term_begin = (int)terms.size();
            for (int j = e.term_begin; j < e.term_end; ++j) {
                if (hte[j].den >= 0) { no("a cashflow term carries its own numeraire (unequal swap tenors)"); break; }
                FTerm ft; ft.w = hte[j].w; ft.atom = fatom(hte[j].atom, t, col_reg, no);
                terms.push_back(ft);
            }
            fe.term_end = (int)terms.size();
            // numeraire identical to the previous event of this date: reuse 1/numeraire
            if (!dl.events[t].empty() && memcmp(&dl.events[t].back().num, &fe.num, sizeof(FAtom)) == 0) fe.flags |= FE_SAME_NUM;
            else fe.flags &= ~FE_SAME_NUM;
            dl.events[t].push_back(fe);
            dl.event_q[t].push_back(q);
        }
    }
}

// stage 3: the numbering of the records ([PV][2 n_dates profiles][CVA] per netting set) and the metric operations of every date
void build_metric_ops(const mcx_book& book, const mcx_fused_desc& d, const int* col_reg, FusedPlan& p, DateLists& dl, Refusal& no)
{
    for (int k = 0; k < MCX_FUSED_MAX_NS; ++k) { p.rec_pv[k] = -1; p.rec_cva[k] = -1; p.lgd[k] = 0.0; }
    for (int k = 0; k < d.n_netting_sets && no.ok; ++k) {
        const mcx_fused_ns_desc& nd = d.ns[k];
        if (nd.netting_set != k) { no("netting-set descriptors must be in order"); break; }
        if (d.want_pv) p.rec_pv[k] = p.n_rec++;
        int rec_prof = -1;
        if (nd.want_profiles) { rec_prof = p.n_rec; p.n_rec += 2 * nd.n_dates; }
        if (nd.want_cva) { p.rec_cva[k] = p.n_rec++; p.lgd[k] = 1.0 - nd.recovery; }
        for (int m = 0; m < nd.n_dates; ++m) {
            const int row = nd.row[m];
            if (row < 0 || row >= d.n_expo_rows) { no("metric row out of range"); break; }
            const int t = d.row_t_idx[row];
            FMetricOp mo;
            memset(&mo, 0, sizeof(mo));
            mo.ns = k; mo.m = m; mo.threshold = nd.threshold;
            mo.rec_profile = nd.want_profiles ? rec_prof + 2 * m : -1;
            mo.has_cva = (nd.want_cva && m < nd.n_dates - 1) ? 1 : 0;
            mo.surv.reg = -1; mo.cond.reg = -1; mo.surv.parts = 0; mo.cond.parts = 0;
            if (mo.has_cva) {
                const int sa = nd.surv_atoms[m], ca = nd.cond_atoms[m];
                if (sa < 0 || sa >= book.n_atoms || ca < 0 || ca >= book.n_atoms) { no("CVA atom out of range"); break; }
                mo.surv = fatom(book.h_atoms[sa], t, col_reg, no);
                mo.cond = fatom(book.h_atoms[ca], t, col_reg, no);
            }
            if (mo.rec_profile >= 0 || mo.has_cva) dl.mops[t].push_back(mo);
        }
    }
}

// ---- stage 4: the FastDate record of one date.  Each piece returns false when the date is not of the straight-line shape; the
// record keeps what was derived up to that point (it is uploaded with valid = 0 and never read).

// the affine part w (a + d x) of a term joins k0 + k1 reg[lin_reg]; false: the date's terms are linear in two registers
bool fold_affine(const FTerm& tm, double& k0, double& k1, int32_t& lin_reg)
{
    k0 += tm.w * tm.atom.a;
    if (tm.atom.d == 0.0) return true;
    const bool one_reg = lin_reg < 0 || lin_reg == tm.atom.reg;
    lin_reg = tm.atom.reg; k1 += tm.w * tm.atom.d;
    return one_reg;
}

// the exercise event of the one two-state product: immediate value (affine part + LeanTerm range, and the book's verified value
// polynomial of the event, mcx_book_collapse_values, copied into this object) against the regression continuation value
bool fast_exercise(const FEvent& e, int q_book, const std::vector<FTerm>& terms, const mcx_book& book, const int* col_reg, FusedPlan& p,
                   FastDate& fd)
{
    if ((fd.flags & (FD_EXERCISE | FD_EXPO)) || e.x.b != 0.0) return false;            // one exercise event, before the exposure
    fd.flags |= FD_EXERCISE;
    fd.ex_term_off = (int32_t)p.lterms.size(); fd.ex_coeff_off = e.coeff_off; fd.ex_strike = e.strike; fd.ex_sign = e.sign;
    fd.ex_x_reg = e.x.reg; fd.ex_x_a = e.x.a; fd.ex_x_d = e.x.d; fd.ex_lin_reg = -1;
    bool ok = true;
    for (int j = e.term_begin; j < e.term_end && ok; ++j) {
        const FTerm& tm = terms[j];
        ok = fold_affine(tm, fd.ex_k0, fd.ex_k1, fd.ex_lin_reg);
        if (tm.atom.b != 0.0) {
            if (tm.atom.reg < 0 || tm.atom.c1 == 0.0) fd.ex_k0 += tm.w * tm.atom.b * exp(tm.atom.c0);      // state-independent term
            else { LeanTerm lt; lt.w = tm.w * tm.atom.b; lt.c0 = tm.atom.c0; lt.c1 = tm.atom.c1; lt.reg = tm.atom.reg; lt.pad = 0; p.lterms.push_back(lt); }
        }
    }
    fd.ex_n = (int32_t)p.lterms.size() - fd.ex_term_off;
    if (!ok) return false;
    const int vq = book.h_event_vpoly.empty() ? -1 : book.h_event_vpoly[q_book];
    if (vq >= 0) {
        const DevVPoly& vp = book.h_vpoly[vq];
        fd.flags |= FD_EX_VPOLY;
        fd.ex_p_lo = vp.lo; fd.ex_p_hi = vp.hi; fd.ex_p_ms = vp.ms; fd.ex_p_ih = vp.ih;
        fd.ex_p_off = (int32_t)p.vcoef.size(); fd.ex_p_blk = vp.n_blk; fd.ex_p_reg = col_reg[vp.col];
        p.vcoef.insert(p.vcoef.end(), book.h_vcoef.begin() + vp.coef_off, book.h_vcoef.begin() + vp.coef_off + (size_t)vp.n_blk * MCX_VPOLY_BLK);
    }
    return true;
}

// a cashflow or a plain option payoff: affine part + at most four exponential terms in the record itself
bool fast_cash(const FEvent& e, const std::vector<FTerm>& terms, FastDate& fd)
{
    fd.flags |= FD_CASH;
    bool ok = true;
    for (int j = e.term_begin; j < e.term_end && ok; ++j) {
        const FTerm& tm = terms[j];
        ok = fold_affine(tm, fd.k0, fd.k1, fd.lin_reg);
        if (tm.atom.b != 0.0) {
            if (fd.n_exp >= 4) return false;
            fd.t_reg[fd.n_exp] = tm.atom.reg; fd.t_w[fd.n_exp] = tm.w * tm.atom.b;
            fd.t_c0[fd.n_exp] = tm.atom.c0; fd.t_c1[fd.n_exp] = tm.atom.c1; fd.n_exp++;
        }
    }
    return ok;
}

// a polynomial exposure: at most two rows in one explanatory variable, or the state-indexed rows of the exercise product alone
bool fast_exposure(const FEvent& e, int n_basis, FastDate& fd, int& n_expo)
{
    const bool stateful = e.sidx >= 0;
    if (e.x.b != 0.0 || n_expo >= 2) return false;
    if ((fd.flags & FD_EXPO) && (fd.x_reg != e.x.reg || fd.x_a != e.x.a || fd.x_d != e.x.d)) return false;
    if (stateful && n_expo > 0) return false;                                          // the state-indexed exposure stands alone
    if (fd.flags & FD_STATE_EXPO) return false;
    fd.flags |= FD_EXPO; fd.x_reg = e.x.reg; fd.x_a = e.x.a; fd.x_d = e.x.d;
    int off = e.coeff_off >= 0 ? e.coeff_off + e.init_state * n_basis : -1;
    if (stateful) { fd.flags |= FD_STATE_EXPO; off = e.coeff_off; if (off < 0) return false; }
    (n_expo == 0 ? fd.coeff_off0 : fd.coeff_off1) = off;
    n_expo++;
    return true;
}

// one event of the date; num: the date's one numeraire so far
bool fast_event(const FEvent& e, int q_book, const std::vector<FTerm>& terms, const mcx_book& book, const int* col_reg, FusedPlan& p,
                FastDate& fd, const FAtom*& num, int& n_expo)
{
    const bool stateful = e.sidx >= 0;
    if (stateful && (e.sidx != 0 || e.n_states != 2)) return false;                    // one two-state product
    const bool plain_option = e.kind == MCX_EV_OPTION && e.aux[0] == 0.0 && !stateful;
    if (e.kind != MCX_EV_CASHFLOW && e.kind != MCX_EV_EXPO_POLY && !plain_option &&
        !(e.kind == MCX_EV_EXERCISE && stateful && e.aux[0] == 0.0)) return false;
    if (stateful && e.kind == MCX_EV_CASHFLOW) return false;
    if ((plain_option || e.kind == MCX_EV_CASHFLOW) && (fd.flags & FD_OPTION)) return false;      // the payoff's max() stands alone
    if (plain_option) {
        if (fd.flags & FD_CASH) return false;
        fd.flags |= FD_OPTION;
        fd.op_strike = e.strike; fd.op_sign = e.sign;
    }
    if (num && memcmp(num, &e.num, sizeof(FAtom)) != 0) return false;                  // one numeraire per date
    num = &e.num;
    if (e.kind == MCX_EV_EXERCISE) return fast_exercise(e, q_book, terms, book, col_reg, p, fd);
    if (e.kind == MCX_EV_CASHFLOW || plain_option) return fast_cash(e, terms, fd);
    return fast_exposure(e, book.n_basis, fd, n_expo);
}

// 1/numeraire of the date's events: a pure exponential of one register, or a constant
bool fast_numeraire(const FAtom& num, FastDate& fd)
{
    if (num.a == 0.0 && num.d == 0.0 && num.b > 0.0) { fd.ni_reg = num.reg; fd.ni_c0 = -num.c0 - log(num.b); fd.ni_c1 = -num.c1; }
    else if (num.b == 0.0 && num.d == 0.0 && num.a != 0.0) { fd.flags |= FD_CONST_NUM; fd.ni_c0 = 1.0 / num.a; }
    else return false;
    return true;
}

// at most one metric operation: its threshold, its EPE / ENE records, its CVA increment (pure-exponential survival)
bool fast_metric_op(const std::vector<FMetricOp>& mops, FastDate& fd)
{
    if (mops.size() > 1) return false;
    if (mops.empty()) return true;
    const FMetricOp& mo = mops[0];
    bool ok = true;
    fd.flags |= FD_METRIC; fd.thr = mo.threshold;
    if (mo.rec_profile >= 0) { fd.flags |= FD_PROFILE; fd.rec_profile = mo.rec_profile; }
    if (mo.has_cva) {
        if (mo.surv.a != 0.0 || mo.surv.d != 0.0 || mo.cond.d != 0.0) ok = false;
        fd.flags |= FD_CVA;
        fd.s_reg = mo.surv.reg; fd.s_b = mo.surv.b; fd.s_c0 = mo.surv.c0; fd.s_c1 = mo.surv.c1;
        fd.c_reg = mo.cond.reg; fd.c_a = mo.cond.a; fd.c_b = mo.cond.b; fd.c_c0 = mo.cond.c0; fd.c_c1 = mo.cond.c1;
    }
    return ok;
}

// merged discount x survival factor of the CVA increment: relu(p / N) S (1 - Sc) = relu(p) (S / N) (1 - Sc) when the date has no
// threshold and records no EPE / ENE profile: one exponential instead of two
void fast_merged_factor(FastDate& fd)
{
    if (!(fd.flags & FD_CVA) || (fd.flags & FD_PROFILE) || fd.thr != 0.0) return;
    fd.flags |= FD_MERGED;
    if (fd.flags & FD_CONST_NUM) { fd.m_b = fd.s_b * fd.ni_c0; fd.m_c0 = fd.s_c0; fd.m_n1 = 0.0; }
    else { fd.m_b = fd.s_b; fd.m_c0 = fd.s_c0 + fd.ni_c0; fd.m_n1 = fd.ni_c1; }
    fd.m_s1 = fd.s_c1;
}

// the straight-line record of date t (valid = 1), for a date of the linear-book shape in a book of one netting set; any other
// date is interpreted from its chunk (valid = 0)
FastDate build_fast_date(int t, const mcx_book& book, const mcx_fused_desc& d, const int* col_reg, const DateLists& dl, FusedPlan& p)
{
    FastDate fd;
    memset(&fd, 0, sizeof(fd));
    fd.ni_reg = fd.lin_reg = fd.x_reg = fd.s_reg = fd.c_reg = -1;
    fd.coeff_off0 = fd.coeff_off1 = -1; fd.rec_profile = -1;
    for (int j = 0; j < 4; ++j) fd.t_reg[j] = -1;
    const std::vector<FMetricOp>& mops = dl.mops[t];
    const FAtom* num = nullptr;
    int n_expo = 0;
    bool ok = d.n_netting_sets == 1;
    for (size_t ei = 0; ei < dl.events[t].size() && ok; ++ei)
        ok = fast_event(dl.events[t][ei], dl.event_q[t][ei], dl.terms[t], book, col_reg, p, fd, num, n_expo);
    if (ok && num) ok = fast_numeraire(*num, fd);
    ok = ok && fast_metric_op(mops, fd);
    if (ok && !num && !mops.empty()) { fd.flags |= FD_CONST_NUM; fd.ni_c0 = 1.0; }      // metric op on an empty date
    // a state reference that is absent (reg < 0) becomes register 0 with a zero coefficient: the kernels may then index the
    // lane's state registers without a range test
    auto bind = [](int32_t& r, double& coef) { if (r < 0) { r = 0; coef = 0.0; } };
    bind(fd.ni_reg, fd.ni_c1); bind(fd.lin_reg, fd.k1); bind(fd.x_reg, fd.x_d); bind(fd.s_reg, fd.s_c1); bind(fd.c_reg, fd.c_c1);
    bind(fd.ex_x_reg, fd.ex_x_d); bind(fd.ex_lin_reg, fd.ex_k1);
    for (int j = 0; j < 4; ++j) bind(fd.t_reg[j], fd.t_c1[j]);
    if (ok) fast_merged_factor(fd);
    if (!ok && (fd.flags & FD_EXERCISE)) p.lterms.resize(fd.ex_term_off);      // the terms of an exercise value that is interpreted after all
    fd.valid = ok ? 1 : 0;
    return fd;
}

// stage 5: the chunks of the interpreted dates (header | events | terms | metric ops, 16-byte aligned) and the size of a wave's
// program slot; a straight-line date is evaluated from its FastDate record by lean_date and has no chunk
void pack_chunks(const DateLists& dl, FusedPlan& p)
{
    const int T = (int)p.fast.size();
    p.date_off.assign(T + 1, 0);
    for (int t = 0; t < T; ++t) {
        p.date_off[t] = (int32_t)p.prog.size();
        if (p.fast[t].valid) continue;
        const std::vector<FEvent>& ev = dl.events[t];
        const std::vector<FTerm>& tm = dl.terms[t];
        const std::vector<FMetricOp>& mo = dl.mops[t];
        ChunkHeader hd;
        hd.n_ev = (int)ev.size(); hd.n_mop = (int)mo.size(); hd.n_terms = (int)tm.size();
        const size_t bytes = sizeof(hd) + sizeof(FEvent) * ev.size() + sizeof(FTerm) * tm.size() + sizeof(FMetricOp) * mo.size();
        const size_t padded = (bytes + 15) & ~(size_t)15;
        hd.bytes = (int32_t)padded;
        const size_t base = p.prog.size();
        p.prog.resize(base + padded, 0);
        unsigned char* dst = p.prog.data() + base;
        memcpy(dst, &hd, sizeof(hd)); dst += sizeof(hd);
        if (hd.n_ev) { memcpy(dst, ev.data(), sizeof(FEvent) * ev.size()); dst += sizeof(FEvent) * ev.size(); }
        if (hd.n_terms) { memcpy(dst, tm.data(), sizeof(FTerm) * tm.size()); dst += sizeof(FTerm) * tm.size(); }
        if (hd.n_mop) memcpy(dst, mo.data(), sizeof(FMetricOp) * mo.size());
        p.max_chunk = std::max(p.max_chunk, (int)padded);
    }
    p.date_off[T] = (int32_t)p.prog.size();
    p.prog.resize(p.prog.size() + 4096, 0);       // slack so the fixed-size prefetch of the last chunk stays in bounds
    // no interpreted date at all: no program slots (NPF = 0, chunk_cap = 0)
    p.npf = p.max_chunk == 0 ? 0 : (p.max_chunk <= 1024 ? 1 : (p.max_chunk <= 2048 ? 2 : 0));
    p.chunk_cap = p.npf > 0 ? p.npf * 1024 : ((p.max_chunk + 255) & ~255);
}

// every date straight-line in a book kf_lean.hip can run
bool straight_line_book(const mcx_sim_desc& sd, const mcx_fused_desc& d, const FusedPlan& p)
{
    bool lean = d.n_netting_sets == 1 && p.n_stateful <= 1;
    for (const FastDate& fd : p.fast) lean = lean && fd.valid != 0;
    // the straight-line kernel skips the zero test under the CIR++ diffusion root: it needs a positive initial intensity (the
    // reference asserts y0 > 0, cirpp.py:40; the state is floored at 1e-12 after every step); other starts run the interpreter
    for (int q = 0; q < sd.n_slots; ++q)
        if (sd.slots[q].kind == MCX_MODEL_CIRPP && !(sd.init_state[sd.slots[q].state_off] > 0.0)) lean = false;
    return lean;
}

// the merged CVA increment and nothing else: what the cva-date kernel evaluates
bool is_cva_increment(const FastDate& fd) { return (fd.flags & (FD_MERGED | FD_EXERCISE | FD_STATE_EXPO)) == FD_MERGED; }

// stage 6: the cva-date kernel of kf_lean.hip: a Vasicek + CIR++ (Euler) CVA book without a PV record whose every date either is the
// merged CVA increment of lean_date (regression exposure of n_basis = 3, no threshold, no EPE / ENE record, no exercise, a
// conditional survival that depends on the state) on the signature's canonical registers, or has no effect on the CVA
void build_cva_dates(const mcx_sim& sim, const mcx_book& book, FusedPlan& p)
{
    const int T = (int)p.fast.size();
    p.cva_dates.resize(T);
    p.cva_only = p.lean && mcx_sim_signature(sim.desc) == SIG_VAS_CIR_E && p.rec_pv[0] < 0 && p.rec_cva[0] >= 0 && book.n_basis == 3;
    for (int t = 0; t < T && p.cva_only; ++t) {
        const FastDate& fd = p.fast[t];
        FastDateCva& c = p.cva_dates[t];
        memset(&c, 0, sizeof(c));
        c.coeff_off0 = c.coeff_off1 = -1;
        if (is_cva_increment(fd)) {
            p.cva_only = fd.c_b != 0.0 && fd.s_reg == FDC_S_REG && fd.ni_reg == FDC_NI_REG && fd.c_reg == FDC_C_REG && fd.x_reg == FDC_X_REG;
            c.m_s1 = fd.m_s1; c.m_n1 = fd.m_n1; c.m_c0 = fd.m_c0; c.m_b = fd.m_b;
            c.c_c1 = fd.c_c1; c.c_c0 = fd.c_c0; c.c_a = fd.c_a; c.c_b = fd.c_b;
            c.x_d = fd.x_d; c.x_a = fd.x_a;
            if (fd.flags & FD_EXPO) { c.coeff_off0 = fd.coeff_off0; c.coeff_off1 = fd.coeff_off1; }
        } else if (fd.flags & (FD_METRIC | FD_EXERCISE | FD_STATE_EXPO)) {
            p.cva_only = false;        // a threshold, an EPE / ENE record or an exercise: the general program
        }
    }
    // The dates after the last CVA increment are all-zero records: each adds +0.0 to the CVA, so the cva-date kernel need not
    // simulate up to them.  cva_steps is the index just past the last sub-step that stores a date with an increment.
    int cva_steps = 0;
    for (size_t k = 0; k < sim.h_steps.size() && p.cva_only; ++k) {
        const int st = sim.h_steps[k].store_idx;
        if (st >= 0 && st < T && is_cva_increment(p.fast[st])) cva_steps = (int)k + 1;
    }
    // (a book without any increment: nothing to stop at, the whole table like every other kernel)
    p.cva_steps = cva_steps > 0 ? cva_steps : (int)sim.h_steps.size();
}

// stage 7, the only one that touches the device: the accepted plan becomes a mcx_fused
int upload(mcx_handle* h, const mcx_sim* sim, const mcx_book* book, const mcx_fused_desc& d, const FusedPlan& p, mcx_fused** out)
{
    mcx_fused* f = new mcx_fused();
    f->sim = sim; f->book = book; f->n_rec = p.n_rec; f->n_ns = d.n_netting_sets; f->n_dates = (int)p.fast.size(); f->n_expo_rows = d.n_expo_rows;
    f->n_stateful = p.n_stateful; f->want_pv = d.want_pv;
    f->npf = p.npf; f->chunk_cap = p.chunk_cap; f->max_chunk = p.max_chunk; f->lean = p.lean ? 1 : 0; f->cva_steps = p.cva_steps;
    for (int k = 0; k < MCX_FUSED_MAX_NS; ++k) { f->rec_pv[k] = p.rec_pv[k]; f->rec_cva[k] = p.rec_cva[k]; f->lgd[k] = p.lgd[k]; }
    for (int q = 0; q < MCX_FUSED_MAX_STATEFUL; ++q) f->init_state[q] = p.init_state[q];
    for (const FastDate& fd : p.fast) { f->date_desc.push_back(fd.valid); f->date_desc.push_back(fd.flags); }
    auto up = [&](auto** dst, const auto& src) -> hipError_t {
        const size_t bytes = sizeof(src[0]) * src.size();
        hipError_t e = hipMalloc((void**)dst, bytes ? bytes : 8);
        if (e != hipSuccess) return e;
        return bytes ? hipMemcpy(*dst, src.data(), bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    f->partial_bytes = sizeof(double) * 4 * (size_t)p.n_rec * 2048;
    hipError_t e = up(&f->d_prog, p.prog);
    if (e == hipSuccess) e = up(&f->d_fast, p.fast);
    if (e == hipSuccess && p.cva_only) e = up(&f->d_cva, p.cva_dates);
    if (e == hipSuccess) e = up(&f->d_lterms, p.lterms);
    if (e == hipSuccess) e = up(&f->d_vcoef, p.vcoef);
    if (e == hipSuccess) e = up(&f->d_date_off, p.date_off);
    if (e == hipSuccess) e = up(&f->d_date_row, p.date_row);
    if (e == hipSuccess) e = hipMalloc(&f->d_partials, f->partial_bytes);
    if (e == hipSuccess) e = hipMalloc(&f->d_out, sizeof(mcx_acc) * (size_t)p.n_rec);
    if (e != hipSuccess) {                                   // nothing leaks: the partially built object is destroyed
        mcx_fused_destroy(f);
        MCX_FAIL(h, -100 - (int)e, "mcx_fused_create: %s", hipGetErrorString(e));
    }
    *out = f;
    return 0;
}

}  // namespace

extern "C" int mcx_fused_create(mcx_handle* h, const mcx_sim* sim, const mcx_book* book, const mcx_fused_desc* d, mcx_fused** out)
{
    if (!h || !sim || !book || !d || !out) return -1;
    MCX_REFUSE_WIDE(h, sim, "mcx_fused_create");
    const mcx_sim_desc& sd = sim->desc;
    if (const int rc = check_arguments(h, sd, book, d)) return rc;
    const int T = sd.n_dates;
    int col_reg[MCX_MAX_STATE];
    state_registers(sd, col_reg);

    FusedPlan p;
    DateLists dl(T);
    Refusal no;
    bucket_events(*book, T, col_reg, p, dl, no);
    p.date_row.assign(T, -1);
    for (int r = 0; r < d->n_expo_rows; ++r) {
        const int t = d->row_t_idx[r];
        if (t < 0 || t >= T) MCX_FAIL(h, -2, "mcx_fused_create: exposure row %d has no timeline date", r);
        p.date_row[t] = r;
    }
    build_metric_ops(*book, *d, col_reg, p, dl, no);
    if (!no.ok) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: %s", no.why.c_str());
    if (p.n_rec < 1) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: no reducible metric requested");
    if ((size_t)9 * p.n_rec * sizeof(double) > 48 * 1024) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: %d records exceed the LDS budget", p.n_rec);

    for (int t = 0; t < T; ++t) p.fast.push_back(build_fast_date(t, *book, *d, col_reg, dl, p));
    p.lterms.resize(p.lterms.size() + 1);          // never empty: the spare term the kernels prefetch
    p.vcoef.resize(p.vcoef.size() + MCX_VPOLY_BLK, 0.0);      // the spare block the kernels prefetch
    pack_chunks(dl, p);
    for (int t = 0; t < T; ++t)
        for (const FEvent& e : dl.events[t])
            if (e.kind == MCX_EV_EXPO_BS) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: analytic Black-Scholes exposures are evaluated by the book kernel (K2)");
    p.lean = straight_line_book(sd, *d, p);
    build_cva_dates(*sim, *book, p);
    // LDS budget: 4 wave slots + the record area (dynamic) must fit comfortably; with kf_fused's static tables (Box-Muller 4 KiB,
    // exponential 1 KiB) a block holds at most 65 KiB of the CU's 160 KiB
    if ((size_t)4 * p.chunk_cap + sizeof(double) * 9 * (size_t)p.n_rec > 60 * 1024)
        MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: a date's event program (%d B) exceeds the per-wave LDS slot budget", p.max_chunk);
    return upload(h, sim, book, *d, p, out);
}

// the one place that decides which kernel a pass runs (fused_run_impl launches it, mcx_fused_describe reports it)
static KfRoute kf_route(const mcx_fused* f, bool inject, bool simulate)
{
    KfRoute r;
    r.kernel = MCX_ROUTE_NONE; r.inject = inject; r.nns = 0; r.nst = 0; r.npf = 0;
    if (f->lean && (simulate || !inject)) { r.kernel = MCX_ROUTE_LEAN; return r; }
    if (inject && !simulate) return r;                        // a paths tensor is never evaluated with injected draws
    r.kernel = MCX_ROUTE_FUSED;
    const bool one_ns = f->n_ns == 1, no_state = f->n_stateful == 0;
    const int npf = (f->npf == 1 || f->npf == 2) ? f->npf : 0;
    if (one_ns && no_state) { r.nns = 1; r.nst = 0; r.npf = npf; }
    else if (one_ns) { r.nns = 1; r.nst = MCX_FUSED_MAX_STATEFUL; r.npf = inject ? 0 : npf; }     // (straight-line dates have no chunk: NNS = 1 runs them)
    else { r.nns = MCX_FUSED_MAX_NS; r.nst = MCX_FUSED_MAX_STATEFUL; r.npf = 0; }
    return r;
}

static int fused_run_impl(mcx_handle* h, const mcx_fused* f, bool simulate, uint64_t seed, uint64_t path_offset, int64_t n_paths,
                          double* d_paths, int64_t ld, double* d_cfs, double* d_expo, int64_t ld_out,
                          const double* d_inject_z, const double* d_inject_u, mcx_acc* h_out, mcx_acc* d_out, void* stream)
{
    // exactly one of h_out (host records, the call synchronises) / d_out (device records, stream-ordered, no synchronisation)
    if (!h || !f || (h_out == nullptr) == (d_out == nullptr)) return -1;
    if (n_paths <= 0) {
        if (h_out) memset(h_out, 0, sizeof(mcx_acc) * (size_t)f->n_rec);
        else MCX_HIP(h, hipMemsetAsync(d_out, 0, sizeof(mcx_acc) * (size_t)f->n_rec, (hipStream_t)stream));
        return 0;
    }
    if ((d_paths || d_inject_z) && ld < n_paths) MCX_FAIL(h, -2, "mcx_fused_run: ld < n_paths");
    if ((d_cfs || d_expo) && ld_out < n_paths) MCX_FAIL(h, -2, "mcx_fused_run: ld_out < n_paths");
    if ((size_t)f->n_rec * sizeof(mcx_acc) > h->pinned_bytes) MCX_FAIL(h, -2, "mcx_fused_run: too many records");
    const mcx_sim_desc& sd = f->sim->desc;
    if (sd.n_uniform && d_inject_z && !d_inject_u) MCX_FAIL(h, -3, "mcx_fused_run: inject_u required with inject_z under QE");
    if (!simulate && (!d_paths || ld < n_paths)) MCX_FAIL(h, -2, "mcx_fused_eval_paths: a paths tensor with ld >= n_paths is required");
    FusedArgs a;
    memset(&a, 0, sizeof(a));
    mcx_fill_k1_args(f->sim, seed, path_offset, n_paths, ld > 0 ? ld : n_paths, d_paths, d_inject_z, d_inject_u, &a.k1);
    // the cva-date kernel computes the CVA records alone: no stored paths, cashflows or exposures
    a.cva_dates = (simulate && !d_inject_z && !d_paths && !d_cfs && !d_expo) ? f->d_cva : nullptr;
    if (a.cva_dates) a.k1.n_steps = f->cva_steps;      // (mcx_launch_kf_lean restores the full count for any other kernel)
    a.prog = f->d_prog; a.fast = f->d_fast; a.lterms = f->d_lterms; a.vcoef = f->d_vcoef; a.date_off = f->d_date_off; a.chunk_cap = f->chunk_cap;
    a.date_row = f->d_date_row; a.coeffs = f->book->d_coeffs; a.cfs = d_cfs; a.expo = d_expo; a.partials = f->d_partials;
    a.ld_out = ld_out; a.n_dates = f->n_dates; a.n_basis = f->book->n_basis; a.n_ns = f->n_ns; a.n_rec = f->n_rec;
    a.n_expo_rows = f->n_expo_rows; a.n_stateful = f->n_stateful;
    for (int k = 0; k < MCX_FUSED_MAX_NS; ++k) { a.rec_pv[k] = f->rec_pv[k]; a.rec_cva[k] = f->rec_cva[k]; a.lgd[k] = f->lgd[k]; }
    for (int k = 0; k < MCX_FUSED_MAX_STATEFUL; ++k) a.init_state[k] = f->init_state[k];
    hipStream_t s = (hipStream_t)stream;
    const bool inj = d_inject_z != nullptr;
    int grid;
    const bool timed = f->timing && (f->t_launch++ % f->timing) == 0 && f->t_count < MCX_FUSED_TIMING_RING;
    if (timed) MCX_HIP(h, hipEventRecord(f->tev[2 * f->t_count], s));
    // host records: the merge writes its few hundred bytes straight into the handle's pinned host buffer (mapped into the
    // device address space): no copy kernel and no extra dispatch on the stream between the pass and its result
    const bool direct = !d_out && sizeof(mcx_acc) * (size_t)f->n_rec <= h->pinned_bytes && h->d_pinned_alias;
    mcx_acc* dst = d_out ? d_out : (direct ? (mcx_acc*)h->d_pinned_alias : f->d_out);
    const KfRoute route = kf_route(f, inj, simulate);
    if (route.kernel == MCX_ROUTE_NONE) MCX_FAIL(h, -2, "mcx_fused_run: no kernel evaluates a paths tensor with injected draws");
    if (route.kernel == MCX_ROUTE_LEAN) {
        // every date is a straight-line record: the two-paths-per-lane kernel of kf_lean.hip (simulating, or streaming a paths tensor)
        // (merging the per-block records in the kernel's last block — arrival ticket + device-scope fences — was measured: the
        //  fences cost ~25 us per launch, three times the kernel boundary they save)
        grid = mcx_launch_kf_lean(a, sd, h->n_cu, inj, simulate, s);
        if (grid < 0) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: (slots=%d, z=%d) has no fused instantiation", sd.n_slots, sd.n_z);
    } else {
        const int64_t tiles = (n_paths + MCX_BLOCK - 1) / MCX_BLOCK;
        grid = (int)std::min<int64_t>(tiles, 2048);
        // keep the tiles-per-block count integral when possible (equal work per block)
        if (tiles > 2048) { int per = (int)((tiles + 2047) / 2048); grid = (int)((tiles + per - 1) / per); }
        const size_t lds = sizeof(double) * (size_t)((9 * f->n_rec + 1) & ~1) + (size_t)4 * f->chunk_cap;
        const bool launched = mcx_dispatch_signature<4>(sd, [&](auto nslot, auto nz, auto sig) {
            launch_kf<decltype(nslot)::value, decltype(nz)::value, decltype(sig)::value>(a, grid, lds, route, simulate, s);
        });
        if (!launched) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "not fusable: (slots=%d, z=%d) has no fused instantiation", sd.n_slots, sd.n_z);
    }
    MCX_HIP(h, hipGetLastError());
    if (timed) { MCX_HIP(h, hipEventRecord(f->tev[2 * f->t_count + 1], s)); ++f->t_count; }
    hipLaunchKernelGGL(kf_merge, dim3(f->n_rec), dim3(MCX_BLOCK), 0, s, f->d_partials, f->n_rec, grid, dst);
    MCX_HIP(h, hipGetLastError());
    if (d_out) return 0;
    if (!direct) MCX_HIP(h, hipMemcpyAsync(h->h_pinned, f->d_out, sizeof(mcx_acc) * (size_t)f->n_rec, hipMemcpyDeviceToHost, s));
    MCX_HIP(h, hipStreamSynchronize(s));
    memcpy(h_out, h->h_pinned, sizeof(mcx_acc) * (size_t)f->n_rec);
    return 0;
}

extern "C" int mcx_fused_is_straight_line(const mcx_fused* f)
{
    return (f && f->lean) ? 1 : 0;
}

extern "C" int mcx_fused_describe(const mcx_fused* f, int32_t inject, int32_t simulate, int32_t* out, int32_t cap)
{
    if (!f || cap < 0 || (cap > 0 && !out)) return -1;
    const int need = MCX_FDESC_HEADER + 2 * f->n_dates;
    if (cap < need) return need;
    const KfRoute r = kf_route(f, inject != 0, simulate != 0);
    int32_t* o = out;
    memset(o, 0, sizeof(int32_t) * MCX_FDESC_HEADER);
    o[MCX_FDESC_LEAN] = f->lean; o[MCX_FDESC_NPF] = f->npf; o[MCX_FDESC_CHUNK_CAP] = f->chunk_cap; o[MCX_FDESC_MAX_CHUNK] = f->max_chunk;
    o[MCX_FDESC_N_NS] = f->n_ns; o[MCX_FDESC_N_STATEFUL] = f->n_stateful; o[MCX_FDESC_N_DATES] = f->n_dates;
    o[MCX_FDESC_CVA_DATES] = f->d_cva != nullptr;
    o[MCX_FDESC_KERNEL] = r.kernel; o[MCX_FDESC_NNS] = r.nns; o[MCX_FDESC_NST] = r.nst; o[MCX_FDESC_KNPF] = r.npf;
    if (f->n_dates > 0) memcpy(o + MCX_FDESC_HEADER, f->date_desc.data(), sizeof(int32_t) * 2 * f->n_dates);
    return need;
}

extern "C" int mcx_fused_run(mcx_handle* h, const mcx_fused* f, uint64_t seed, uint64_t path_offset, int64_t n_paths,
                             double* d_paths, int64_t ld, double* d_cfs, double* d_expo, int64_t ld_out,
                             const double* d_inject_z, const double* d_inject_u, mcx_acc* h_out, void* stream)
{
    return fused_run_impl(h, f, true, seed, path_offset, n_paths, d_paths, ld, d_cfs, d_expo, ld_out, d_inject_z, d_inject_u, h_out, nullptr, stream);
}

extern "C" int mcx_fused_run_device(mcx_handle* h, const mcx_fused* f, uint64_t seed, uint64_t path_offset, int64_t n_paths,
                                    double* d_paths, int64_t ld, double* d_cfs, double* d_expo, int64_t ld_out,
                                    const double* d_inject_z, const double* d_inject_u, mcx_acc* d_out, void* stream)
{
    return fused_run_impl(h, f, true, seed, path_offset, n_paths, d_paths, ld, d_cfs, d_expo, ld_out, d_inject_z, d_inject_u, nullptr, d_out, stream);
}

extern "C" int mcx_fused_eval_paths(mcx_handle* h, const mcx_fused* f, const double* d_paths, int64_t n_paths, int64_t ld,
                                    double* d_cfs, double* d_expo, int64_t ld_out, mcx_acc* h_out, void* stream)
{
    return fused_run_impl(h, f, false, 0, 0, n_paths, const_cast<double*>(d_paths), ld, d_cfs, d_expo, ld_out, nullptr, nullptr, h_out, nullptr, stream);
}

extern "C" int mcx_fused_eval_paths_device(mcx_handle* h, const mcx_fused* f, const double* d_paths, int64_t n_paths, int64_t ld,
                                           double* d_cfs, double* d_expo, int64_t ld_out, mcx_acc* d_out, void* stream)
{
    return fused_run_impl(h, f, false, 0, 0, n_paths, const_cast<double*>(d_paths), ld, d_cfs, d_expo, ld_out, nullptr, nullptr, nullptr, d_out, stream);
}
