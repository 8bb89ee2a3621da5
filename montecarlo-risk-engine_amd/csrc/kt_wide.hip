// kt_wide.hip — dual paths of a WIDE model (mcx_sim_create_wide: up to MCX_WIDE_MAX_SLOTS correlated one-factor sub-models), one state
// column per block row (gfx950 / CDNA4, wave64).
//
// The narrow dual path kernels (kt_book.hip kt_paths / kt_paths_chol) give one lane one path of the WHOLE model: z[], every state and
// its MCX_TANGENT_NP tangents stay in registers.  At 32 slots that is (1 + NP) images of 64 state doubles next to a primal kernel that
// already sits at 255 VGPRs.  This kernel needs none of it, because of two facts about a wide model:
//   1. its sub-models are one-factor and independent given their correlated normal: the state of slot r at every date is a function
//      of the parameters of slot r and of zc_r = sum_{c <= r} L[r][c] z[c] alone;
//   2. the tangent of slot r's state with respect to a parameter is non-zero only where that parameter reaches the slot's OWN
//      descriptor numbers: its dslot row, its dinit rows, its daux rows and, under ANALYTICAL, row r of the factors' tangents.
// A chunk of NP parameters therefore touches a few slots (all of them only for the shared rate of BlackScholesMulti): the dual path
// tensor is sparse by columns.  The grid is (ceil(n / MCX_BLOCK), n_active); blockIdx.y picks a slot r from the device list of the
// ACTIVE slots (built on the host from the tables), and one lane owns one path of that one slot:
//   * slot record, dslot / dinit / daux rows: wave-uniform scalar loads at the point of use (ld_dual of mcx_dual_step.h);
//   * zc_r is formed by STREAMING the draws: for q = 0 .. r >> 1 one draw_pair<true, 7, true> on the counters (path, sub-step, q) —
//     k1_paths_wide's call — or the injected block, accumulated as k1_paths_wide accumulates (L[r][0] z[0], then fma ascending in c;
//     EULER row 0 is z[0] itself; an odd row end drops the pair's second normal).  No z[] array, nothing indexed at run time;
//   * ANALYTICAL: zc is a dual number, the factor's row r carries its tangent (ktp_fma of mcx_dual_step.h); EULER: a plain double (the
//     correlations are not model parameters);
//   * the dual step of the slot's kind is the narrow kernels' own: dual_step_euler / dual_step_analytical of mcx_dual_step.h, which
//     kt_paths and kt_paths_chol call too, here with the slot parameters read from the device table (DualTable) where the narrow
//     kernels read the kernel-argument segment (DualKarg).  ld_dual and ktp_fma live there as well.  Sharing left every kernel of
//     kt_book.hip instruction for instruction as it was, and this kernel's four instantiations identical (INJECT) or with the same
//     opcode sequence under other register names (Philox): profiles/dual_step_asm_compare.md.  The two Hull-White steps (no narrow
//     kernel has them) sit behind the maps' HW flag, set only in the instantiations which mcx_tangent_paths_wide_hw launches for a
//     sim that holds a Hull-White slot: the plain instantiations keep the instruction stream they had without them.
//     NOT shared, on purpose: the prologue of kt_paths / kt_paths_chol (initial state, draws) is still written out in both — one
//     function for the initial-state loop changed the code of all 16 of their instantiations, one for the draw loop 10 of them;
//   * only the TANGENT images of the slot's state columns are written (c, and c + 1 unless Black-Scholes: wide_store's placement).  The
//     value image is the primal kernel's (mcx_wide_generate), so image 0 is K1's bytes; the columns of inactive slots stay at the
//     zero the entry point's memset wrote.
// The price is redundant draws: a block row of slot r redraws (r >> 1) + 1 Philox pairs per sub-step, a chunk with active slots A
// costs sum_{r in A} ((r >> 1) + 1) pairs per path-step against n_slots / 2 of one primal run.
#include <algorithm>

#include "mcx_dual_step.h"

namespace {

struct KTWArgs {
    const mcx_slot* __restrict__ slots;        // device [n_slots] (mcx_sim::d_slots)
    const double* __restrict__ init_state;     // device [n_state]
    const mcx_step* __restrict__ steps;
    const double* __restrict__ chol;
    const double* __restrict__ aux;
    const double* __restrict__ dslot;          // [n_slots][MCX_SLOT_NPARAM][NP]
    const double* __restrict__ dinit;          // [n_state][NP]
    const double* __restrict__ daux;           // [n_steps][n_slots][MCX_AUX][NP]
    const double* __restrict__ dchol;          // [n_chol][n_slots][n_slots][NP], ANALYTICAL only
    const int32_t* __restrict__ active;        // device [gridDim.y]: the active slots, ascending
    double* __restrict__ dpaths;               // [NP][T][D][ld]
    const double* __restrict__ inject_z;       // [n_steps][n_slots][ld]
    int64_t n, ld, pstride;                    // pstride = T * D * ld
    uint64_t seed, path_offset;
    int32_t scheme, n_steps, n_state, n_slots, n_initial_store, pad;
};

// the tangent images of one state column at stored date t
__device__ __forceinline__ void ktw_store(const KTWArgs& a, int t, int col, int64_t i, const DN& x)
{
    const int64_t off = ((int64_t)t * a.n_state + col) * a.ld + i;
#pragma unroll
    for (int q = 0; q < NP; ++q) a.dpaths[q * a.pstride + off] = x.d[q];
}

// HW: the instantiation that also holds the two Hull-White dual steps (mcx_tangent_paths_wide_hw launches it for a sim with a
// Hull-White slot, and only for such a sim); without it the kernel is the one it was before those steps existed
template <bool INJECT, bool HW>
__global__ __launch_bounds__(MCX_BLOCK) void kt_paths_wide(const KTWArgs a)
{
    __shared__ double bm_lds[INJECT ? 2 : MCX_BM_LDS_DOUBLES];
    if (!INJECT) mcx_bm_load(bm_lds);
    const double* tab = bm_lds;
    const int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int r = ldk(a.active + blockIdx.y);                       // this block row's slot: wave-uniform
    const int ns = a.n_slots;
    const mcx_slot* __restrict__ sl = a.slots + r;
    const int kind = ldk(&sl->kind), col = ldk(&sl->state_off);
    const bool bs = kind == MCX_MODEL_BS;
    const double* __restrict__ p = sl->p;
    const double* __restrict__ dp = a.dslot + (int64_t)r * MCX_SLOT_NPARAM * NP;
    const uint64_t path = a.path_offset + (uint64_t)i;
    DN s0 = ld_dual(ldk(a.init_state + col), a.dinit + (int64_t)col * NP);
    DN s1 = bs ? dconst<NP>(0.0) : ld_dual(ldk(a.init_state + col + 1), a.dinit + (int64_t)(col + 1) * NP);
    for (int t = 0; t < a.n_initial_store; ++t) {
        ktw_store(a, t, col, i, s0);
        if (!bs) ktw_store(a, t, col + 1, i, s1);
    }
    const mcx_bm_coef bc = mcx_bm_coef_load();
    const mcx_bm_vconst vc = mcx_bm_vconst_make(bc);
    const bool euler = a.scheme == MCX_SCHEME_EULER;
    const int last = r >> 1;                                         // the Philox pair that holds z[r]
#pragma unroll 1
    for (int step = 0; step < a.n_steps; ++step) {
        const mcx_step sp = ldk_struct(&a.steps[step]);
        // EULER: the one factor of the correlation matrix (mcx_sim_create_wide checks chol_idx == 0), whose first entry is 1
        const int64_t row = ((int64_t)(euler ? 0 : sp.chol_idx) * ns + r) * ns;
        const double* __restrict__ Lr = a.chol + row;
        const double* __restrict__ dLr = a.dchol + row * NP;         // (read under ANALYTICAL only)
        double zv = 0.0;                                             // zc_r under EULER
        DN zd = dconst<NP>(0.0);                                     // zc_r under ANALYTICAL: the factor's row carries a tangent
#pragma unroll 1
        for (int q = 0; q <= last; ++q) {
            const int c0 = 2 * q;
            const bool both = c0 + 1 <= r;                           // an odd row end drops the pair's second normal
            double z0, z1 = 0.0;
            if (INJECT) {
                z0 = a.inject_z[((int64_t)step * ns + c0) * a.ld + i];
                if (both) z1 = a.inject_z[((int64_t)step * ns + c0 + 1) * a.ld + i];
            } else {
                double ua;
                draw_pair<true, 7, true>(a.seed, path, (uint32_t)step, (uint32_t)q, ua, z0, z1, tab, bc, &vc);
            }
            if (euler) {
                if (q == 0) zv = r == 0 ? z0 : ldk(Lr) * z0;
                else zv = fma(ldk(Lr + c0), z0, zv);
                if (both) zv = fma(ldk(Lr + c0 + 1), z1, zv);
            } else {
                zd = ktp_fma(ld_dual(ldk(Lr + c0), dLr + (int64_t)c0 * NP), z0, zd);
                if (both) zd = ktp_fma(ld_dual(ldk(Lr + c0 + 1), dLr + (int64_t)(c0 + 1) * NP), z1, zd);
            }
        }
        const DualTable ps{p, dp};
        const DualTable ax{a.aux + ((int64_t)step * ns + r) * MCX_AUX, a.daux + ((int64_t)step * ns + r) * MCX_AUX * NP};
        if (euler) dual_step_euler<HW>(kind, ps, ax, sp.dt, sp.sqrt_dt, zv, s0, s1);
        else dual_step_analytical<HW>(bs, kind, ps, ax, sp.dt, zd, s0, s1);
        const int st = sp.store_idx;
        if (st >= 0) {
            ktw_store(a, st, col, i, s0);
            if (!bs) ktw_store(a, st, col + 1, i, s1);
        }
    }
}

// any entry of v[0 .. n) non-zero (a NaN counts: it must reach the images)
bool ktw_any(const double* v, size_t n)
{
    for (size_t q = 0; q < n; ++q)
        if (!(v[q] == 0.0)) return true;
    return false;
}

// mcx_tangent_paths_wide and mcx_tangent_paths_wide_hw.  allow_hw: the latter, which also takes Hull-White slots under both schemes.
// Every check comes before the first upload: a refused call enqueues nothing and writes nothing.
int ktw_tangent_paths_wide(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux,
                           const double* h_dchol, uint64_t seed, uint64_t path_offset, int64_t n_paths, double* d_paths, double* d_dpaths,
                           int64_t ld, const double* d_inject_z, int32_t* n_active_out, void* stream, const char* who, bool allow_hw)
{
    if (int rc = mcx_tangent_check_args(h, sim, h_dslot, h_dinit, h_daux, h_dchol, 1u << MCX_SCHEME_ANALYTICAL, d_paths, d_dpaths, n_paths, ld,
                                        who, true, nullptr)) {
        if (rc > 0 && n_active_out) *n_active_out = 0;
        return rc > 0 ? 0 : rc;
    }
    const mcx_sim_desc& sd = sim->desc;
    const bool euler = sd.scheme == MCX_SCHEME_EULER, analytic = sd.scheme == MCX_SCHEME_ANALYTICAL;
    if (!euler && !analytic) MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: scheme %d: EULER or ANALYTICAL scheme only", who, (int)sd.scheme);
    const int ns = sd.n_slots;
    if (ns < 1 || ns > MCX_WIDE_MAX_SLOTS || sd.n_z != ns || (int)sim->h_slots.size() != ns)
        MCX_FAIL(h, MCX_E_NOT_FUSABLE, "%s: one normal per slot and 1 .. %d slots expected", who, MCX_WIDE_MAX_SLOTS);
    bool has_hw = false;
    if (int rc = mcx_tangent_check_kinds(h, who, sim->h_slots.data(), ns, analytic, allow_hw, &has_hw)) return rc;
    // the kernel indexes the factors and the dates by the steps' records
    if (int rc = mcx_tangent_check_steps(h, who, sim, sd.n_chol, true)) return rc;
    // the active slots: those a non-zero entry of the tables reaches
    int32_t active[MCX_WIDE_MAX_SLOTS];
    int n_active = 0;
    for (int r = 0; r < ns; ++r) {
        const int c = sim->h_slots[r].state_off, dim = mcx_kind_state_dim(sim->h_slots[r].kind);
        bool on = ktw_any(h_dslot + (size_t)r * MCX_SLOT_NPARAM * NP, (size_t)MCX_SLOT_NPARAM * NP) || ktw_any(h_dinit + (size_t)c * NP, (size_t)dim * NP);
        for (int k = 0; k < sd.n_steps && !on; ++k) on = ktw_any(h_daux + ((size_t)k * ns + r) * MCX_AUX * NP, (size_t)MCX_AUX * NP);
        for (int f = 0; analytic && f < sd.n_chol && !on; ++f) on = ktw_any(h_dchol + ((size_t)f * ns + r) * ns * NP, (size_t)ns * NP);
        if (on) active[n_active++] = r;
    }
    hipStream_t s = (hipStream_t)stream;
    // the tables go up before anything is written: a failed upload leaves the outputs untouched too
    KTWArgs a;
    memset(&a, 0, sizeof(a));
    if (n_active > 0) {
        mcx_tangent_tables t;
        if (int rc = mcx_tangent_upload(h, sd, h_dslot, h_dinit, h_daux, analytic ? h_dchol : nullptr, s, &t)) return rc;
        a.dslot = t.dslot; a.dinit = t.dinit; a.daux = t.daux;
        a.dchol = analytic ? t.dchol : t.dslot;            // (EULER: never read)
        a.active = (const int32_t*)mcx_stage_small(h, active, sizeof(int32_t) * (size_t)n_active, s);
        if (!a.active) return -100;
    }
    // the value image: the primal kernel, so image 0 is K1's bytes and a frozen exercise policy sees the base run's values
    const int rc = mcx_wide_generate(h, sim, seed, path_offset, n_paths, ld, nullptr, d_paths, d_inject_z, stream);
    if (rc) return rc;
    const int64_t rows = (int64_t)NP * sd.n_dates * sd.n_state;
    if (ld == n_paths) MCX_HIP(h, hipMemsetAsync(d_dpaths, 0, sizeof(double) * (size_t)rows * (size_t)ld, s));
    else MCX_HIP(h, hipMemset2DAsync(d_dpaths, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)n_paths, (size_t)rows, s));   // the padding stays
    if (n_active > 0) {
        a.slots = sim->d_slots; a.init_state = sim->d_init; a.steps = sim->d_steps; a.chol = sim->d_chol; a.aux = sim->d_aux;
        a.dpaths = d_dpaths; a.inject_z = d_inject_z;
        a.n = n_paths; a.ld = ld; a.pstride = (int64_t)sd.n_dates * sd.n_state * ld;
        a.seed = seed; a.path_offset = path_offset;
        a.scheme = sd.scheme; a.n_steps = sd.n_steps; a.n_state = sd.n_state; a.n_slots = ns; a.n_initial_store = sd.n_initial_store;
        const dim3 grid((unsigned)((n_paths + MCX_BLOCK - 1) / MCX_BLOCK), (unsigned)n_active);
        if (has_hw) {
            if (d_inject_z) hipLaunchKernelGGL((kt_paths_wide<true, true>), grid, dim3(MCX_BLOCK), 0, s, a);
            else hipLaunchKernelGGL((kt_paths_wide<false, true>), grid, dim3(MCX_BLOCK), 0, s, a);
        } else if (d_inject_z) hipLaunchKernelGGL((kt_paths_wide<true, false>), grid, dim3(MCX_BLOCK), 0, s, a);
        else hipLaunchKernelGGL((kt_paths_wide<false, false>), grid, dim3(MCX_BLOCK), 0, s, a);
        MCX_HIP(h, hipGetLastError());
    }
    MCX_HIP(h, hipStreamSynchronize(s));
    if (n_active_out) *n_active_out = n_active;
    return 0;
}

}  // namespace

extern "C" int mcx_tangent_paths_wide(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux,
                                      const double* h_dchol, uint64_t seed, uint64_t path_offset, int64_t n_paths, double* d_paths,
                                      double* d_dpaths, int64_t ld, const double* d_inject_z, int32_t* n_active_out, void* stream)
{
    return ktw_tangent_paths_wide(h, sim, h_dslot, h_dinit, h_daux, h_dchol, seed, path_offset, n_paths, d_paths, d_dpaths, ld, d_inject_z,
                                  n_active_out, stream, "mcx_tangent_paths_wide", false);
}

// mcx_tangent_paths_wide that also takes Hull-White slots (EULER and ANALYTICAL); on a sim without one it is mcx_tangent_paths_wide
extern "C" int mcx_tangent_paths_wide_hw(mcx_handle* h, const mcx_sim* sim, const double* h_dslot, const double* h_dinit, const double* h_daux,
                                         const double* h_dchol, uint64_t seed, uint64_t path_offset, int64_t n_paths, double* d_paths,
                                         double* d_dpaths, int64_t ld, const double* d_inject_z, int32_t* n_active_out, void* stream)
{
    return ktw_tangent_paths_wide(h, sim, h_dslot, h_dinit, h_daux, h_dchol, seed, path_offset, n_paths, d_paths, d_dpaths, ld, d_inject_z,
                                  n_active_out, stream, "mcx_tangent_paths_wide_hw", true);
}
