// k1_wide.hip — K1 for wide models: 9 .. MCX_WIDE_MAX_SLOTS correlated one-factor sub-models (gfx950 / CDNA4, wave64).
//
// The contract is k1_paths' (k1_paths.hip), extended to n_z = n_slots <= 32: the same Philox counters (path, sub-step, draw = f >> 1),
// the same guarded table-driven Box-Muller pair, the same ascending-fma Cholesky rows, the same step maps (step_slot of mcx_device.h,
// run-time scheme), the same stores.  What differs is where the model lives:
//   * k1_paths<NSLOT, ...> carries every slot record in the kernel-argument segment and keeps it in SGPRs for the whole run: at
//     5-8 generic slots that is already 175-300 SGPR spills.  Here the slot records sit in a DEVICE TABLE (mcx_sim::d_slots) and every
//     field is a wave-uniform scalar load at its point of use, like the factor and the aux rows: nothing model-sized stays live.
//   * one lane owns one path; z[CAP] and the state reg[2 CAP] are register arrays with COMPILE-TIME indices only (every slot loop is
//     fully unrolled, the run-time slot count is a wave-uniform early exit `s >= n_slots`), so nothing is indexed at run time and
//     nothing goes to scratch.  Two capacities are instantiated, 16 and 32 slots: a 12-factor model does not pay for 32.
//   * the correlated normal of row r is consumed by slot r as soon as it is formed (n_z == n_slots, z_off == slot): there is no
//     zc[] array, only z[] stays live across the rows.
//   * the kind switch names the five kinds a wide model may hold and calls step_slot<KIND, -1>: the same case bodies the generic
//     narrow kernel runs, without 32 copies of the Heston and Schwartz maps that a wide model cannot contain.
#include "mcx_device.h"

namespace {

struct WideArgs {
    const mcx_slot* __restrict__ slots;        // device [n_slots]
    const double* __restrict__ init_state;     // device [n_state]
    const mcx_step* __restrict__ steps;
    const double* __restrict__ chol;
    const double* __restrict__ aux;
    double* __restrict__ paths;
    const double* __restrict__ inject_z;       // [n_steps][n_slots][ld]
    const double* __restrict__ init_paths;     // nullable: per-path initial state [n_state][ld]
    int64_t n, ld;
    uint64_t seed, path_offset;
    int32_t scheme, n_steps, n_state, n_slots, n_initial_store, flags;
};

// a slot record as step_slot reads it: the parameters through the constant address space (scalar loads at the point of use)
struct WideSlotView {
    const MCX_KONST double* p;
    int kind;                                  // (named by step_slot's run-time dispatch only: the callers here fix KIND)
};

// A table pointer the optimiser cannot see through.  The slot records and (under EULER) the factor do not change from one sub-step
// to the next, so the loop-invariant-code pass would hoist their several hundred scalar loads out of the sub-step loop and keep the
// values in SGPRs — which do not exist: they would be spilled.  Re-deriving the pointer per sub-step keeps each load at its use.
template <class T>
__device__ __forceinline__ const T* wide_opaque(const T* p)
{
    asm volatile("" : "+s"(p));
    return p;
}

// The same for the slot count: every guard `s < n_slots` of the unrolled loops is the same comparison, and its 32 results would be
// kept as 64-bit masks (and spilled) for the whole kernel.  Each code region compares against its own copy: s_cmp + s_cbranch.
__device__ __forceinline__ int wide_opaque(int v)
{
    asm volatile("" : "+s"(v));
    return v;
}

template <int CAP>
__device__ __forceinline__ void wide_store(const WideArgs& a, int t, int64_t i, const double (&reg)[2 * CAP])
{
    const int64_t D = a.n_state;
    const int ns = wide_opaque(a.n_slots);
    const mcx_slot* slots = wide_opaque(a.slots);
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        if (s < ns) {
            const int kind = ldk(&slots[s].kind), c = ldk(&slots[s].state_off);
            a.paths[((int64_t)t * D + c) * a.ld + i] = reg[2 * s];
            if (kind != MCX_MODEL_BS) a.paths[((int64_t)t * D + c + 1) * a.ld + i] = reg[2 * s + 1];
        }
    }
}

template <int CAP, bool INJECT>
__global__ __launch_bounds__(MCX_BLOCK) void k1_paths_wide(const WideArgs a)
{
    static_assert(CAP % 2 == 0 && CAP <= MCX_WIDE_MAX_SLOTS, "capacity");
    __shared__ double bm_lds[INJECT ? 2 : MCX_BM_LDS_DOUBLES];
    if (!INJECT) mcx_bm_load(bm_lds);
    const double* tab = bm_lds;
    const int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int ns = a.n_slots;
    const uint64_t path = a.path_offset + (uint64_t)i;
    double reg[2 * CAP];
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        reg[2 * s] = 0.0; reg[2 * s + 1] = 0.0;
        if (s < ns) {
            const int kind = ldk(&a.slots[s].kind), c = ldk(&a.slots[s].state_off);
            if (a.init_paths) {
                reg[2 * s] = a.init_paths[(int64_t)c * a.ld + i];
                if (kind != MCX_MODEL_BS) reg[2 * s + 1] = a.init_paths[(int64_t)(c + 1) * a.ld + i];
            } else {
                reg[2 * s] = ldk(a.init_state + c);
                if (kind != MCX_MODEL_BS) reg[2 * s + 1] = ldk(a.init_state + c + 1);
            }
        }
    }
    for (int t = 0; t < a.n_initial_store; ++t) wide_store<CAP>(a, t, i, reg);
    const mcx_bm_coef bc = mcx_bm_coef_load();
    const mcx_bm_vconst vc = mcx_bm_vconst_make(bc);
    const bool euler = a.scheme == MCX_SCHEME_EULER;
    for (int k = 0; k < a.n_steps; ++k) {
        const int ns = wide_opaque(a.n_slots);
        double z[CAP];
        // the normals: component f & 1 of the pair of Philox block (path, k, f >> 1); an odd count discards the last z1
#pragma unroll
        for (int q = 0; q < CAP / 2; ++q) {
            z[2 * q] = 0.0; z[2 * q + 1] = 0.0;
            if (2 * q < ns) {
                if (INJECT) {
                    z[2 * q] = a.inject_z[((int64_t)k * ns + 2 * q) * a.ld + i];
                    if (2 * q + 1 < ns) z[2 * q + 1] = a.inject_z[((int64_t)k * ns + 2 * q + 1) * a.ld + i];
                } else {
                    double ua, z0, z1;
                    draw_pair<true, 7, true>(a.seed, path, (uint32_t)k, (uint32_t)q, ua, z0, z1, tab, bc, &vc);
                    z[2 * q] = z0; z[2 * q + 1] = z1;
                }
            }
        }
        const mcx_step sp = ldk_struct(&a.steps[k]);
        // EULER: the one factor of the correlation matrix (mcx_sim_create_wide checks chol_idx == 0), whose first entry is 1
        const double* __restrict__ L = wide_opaque(euler ? a.chol : a.chol + (int64_t)sp.chol_idx * ns * ns);
        const mcx_slot* slots = wide_opaque(a.slots);
        const double* __restrict__ ax = a.aux + (int64_t)k * ns * MCX_AUX;
#pragma unroll
        for (int r = 0; r < CAP; ++r) {
            if (r >= ns) continue;
            const double* __restrict__ Lr = L + r * ns;
            double zc = ldk(Lr) * z[0];
            if (r == 0 && euler) zc = z[0];
#pragma unroll
            for (int c = 1; c <= r; ++c) zc = fma(ldk(Lr + c), z[c], zc);
            const mcx_slot* sl = slots + r;
            const WideSlotView sv{(const MCX_KONST double*)(uintptr_t)sl->p, 0};
            const int fl = a.flags | ldk(&sl->flags);
            const AuxPtr au = aux_of_slot(ax, r);
            double& s0 = reg[2 * r];
            double& s1 = reg[2 * r + 1];
            switch (ldk(&sl->kind)) {
            case MCX_MODEL_BS: step_slot<MCX_MODEL_BS, -1>(sv, a.scheme, fl, sp.dt, sp.sqrt_dt, au, s0, s1, zc, 0.0, 0.0); break;
            case MCX_MODEL_VASICEK: step_slot<MCX_MODEL_VASICEK, -1>(sv, a.scheme, fl, sp.dt, sp.sqrt_dt, au, s0, s1, zc, 0.0, 0.0); break;
            case MCX_MODEL_HW: step_slot<MCX_MODEL_HW, -1>(sv, a.scheme, fl, sp.dt, sp.sqrt_dt, au, s0, s1, zc, 0.0, 0.0); break;
            case MCX_MODEL_CIRPP: step_slot<MCX_MODEL_CIRPP, -1>(sv, a.scheme, fl, sp.dt, sp.sqrt_dt, au, s0, s1, zc, 0.0, 0.0); break;
            case MCX_MODEL_CIRPP_DET: step_slot<MCX_MODEL_CIRPP_DET, -1>(sv, a.scheme, fl, sp.dt, sp.sqrt_dt, au, s0, s1, zc, 0.0, 0.0); break;
            default: break;
            }
        }
        if (sp.store_idx >= 0) wide_store<CAP>(a, sp.store_idx, i, reg);
    }
}

template <int CAP>
void launch_wide(const WideArgs& a, bool inject, hipStream_t s)
{
    const int grid = (int)((a.n + MCX_BLOCK - 1) / MCX_BLOCK);
    if (inject) hipLaunchKernelGGL((k1_paths_wide<CAP, true>), dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((k1_paths_wide<CAP, false>), dim3(grid), dim3(MCX_BLOCK), 0, s, a);
}

}  // namespace

extern "C" int mcx_sim_create_wide(mcx_handle* h, const mcx_wide_sim_desc* d, mcx_sim** out)
{
    if (!h || !d || !out) return -1;
    if (d->n_slots < 1 || d->n_slots > MCX_WIDE_MAX_SLOTS || d->n_z != d->n_slots || d->n_state > MCX_WIDE_MAX_STATE || d->n_uniform != 0 || !d->slots)
        MCX_FAIL(h, -2, "mcx_sim_create_wide: dimensions out of range (slots %d, z %d, state %d): 1 .. MCX_WIDE_MAX_SLOTS = %d one-factor slots",
                 d->n_slots, d->n_z, d->n_state, MCX_WIDE_MAX_SLOTS);
    if (int rc = mcx_sim_check_slots(h, "mcx_sim_create_wide", d->slots, d->n_slots, d->n_state, d->scheme, true)) return rc;
    if (int rc = mcx_sim_check_steps(h, "mcx_sim_create_wide", d->steps, d->n_steps, d->n_dates, d->n_chol, d->scheme)) return rc;
    MCX_HIP(h, hipSetDevice(h->device));
    mcx_sim* sim = new mcx_sim();
    memset(&sim->desc, 0, sizeof(sim->desc));          // desc.slots stays empty: every reader checks `wide` first
    sim->desc.scheme = d->scheme; sim->desc.n_slots = d->n_slots; sim->desc.n_state = d->n_state; sim->desc.n_z = d->n_z;
    sim->desc.n_steps = d->n_steps; sim->desc.n_dates = d->n_dates; sim->desc.n_chol = d->n_chol;
    sim->desc.n_initial_store = d->n_initial_store; sim->desc.flags = d->flags;
    sim->wide = true;
    sim->d_steps = nullptr; sim->d_chol = nullptr; sim->d_aux = nullptr; sim->d_slots = nullptr; sim->d_init = nullptr;
    sim->n_state_total = d->n_state;
    sim->h_steps.assign(d->steps, d->steps + (d->n_steps > 0 ? d->n_steps : 0));
    sim->h_slots.assign(d->slots, d->slots + d->n_slots);
    const int ns = d->n_slots;
    const size_t n_steps = (size_t)(d->n_steps > 0 ? d->n_steps : 0);
    hipError_t e = hipMalloc(&sim->d_steps, sizeof(mcx_step) * (n_steps ? n_steps : 1));
    if (e == hipSuccess) e = hipMalloc(&sim->d_chol, sizeof(double) * (size_t)(d->n_chol > 0 ? d->n_chol : 1) * ns * ns);
    if (e == hipSuccess) e = hipMalloc(&sim->d_aux, sizeof(double) * (n_steps ? n_steps : 1) * ns * MCX_AUX);
    if (e == hipSuccess) e = hipMalloc(&sim->d_slots, sizeof(mcx_slot) * ns);
    if (e == hipSuccess) e = hipMalloc(&sim->d_init, sizeof(double) * (size_t)d->n_state);
    if (e == hipSuccess) e = hipMemcpy(sim->d_slots, d->slots, sizeof(mcx_slot) * ns, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        e = hipMemcpy(sim->d_init, d->init_state, sizeof(double) * (size_t)d->n_state, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && n_steps) e = hipMemcpy(sim->d_steps, d->steps, sizeof(mcx_step) * n_steps, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_steps) {
        const std::vector<double> aux = mcx_sim_device_aux(d->slots, ns, d->steps, (int)n_steps, d->aux, d->scheme);
        e = hipMemcpy(sim->d_aux, aux.data(), sizeof(double) * aux.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && d->n_chol > 0)
        e = hipMemcpy(sim->d_chol, d->chol, sizeof(double) * (size_t)d->n_chol * ns * ns, hipMemcpyHostToDevice);
    if (e != hipSuccess) {                      // nothing of a failed create survives
        h->err = std::string("mcx_sim_create_wide: ") + hipGetErrorString(e);
        mcx_sim_destroy(sim);
        return -100;
    }
    *out = sim;
    return 0;
}

// the launch of mcx_generate_paths / mcx_generate_paths_from_state for a wide sim (k1_paths.hip checks the arguments)
int mcx_wide_generate(mcx_handle* h, const mcx_sim* sim, uint64_t seed, uint64_t path_offset, int64_t n_paths, int64_t ld,
                      const double* d_init_state, double* d_paths, const double* d_inject_z, void* stream)
{
    const mcx_sim_desc& d = sim->desc;
    WideArgs a;
    memset(&a, 0, sizeof(a));
    a.slots = sim->d_slots; a.init_state = sim->d_init; a.steps = sim->d_steps; a.chol = sim->d_chol; a.aux = sim->d_aux;
    a.paths = d_paths; a.inject_z = d_inject_z; a.init_paths = d_init_state;
    a.n = n_paths; a.ld = ld; a.seed = seed; a.path_offset = path_offset;
    a.scheme = d.scheme; a.n_steps = d.n_steps; a.n_state = d.n_state; a.n_slots = d.n_slots;
    a.n_initial_store = d.n_initial_store; a.flags = d.flags;
    if (d.n_slots <= 16) launch_wide<16>(a, d_inject_z != nullptr, (hipStream_t)stream);
    else launch_wide<32>(a, d_inject_z != nullptr, (hipStream_t)stream);
    MCX_HIP(h, hipGetLastError());
    return 0;
}
