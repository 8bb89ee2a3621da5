// k4_fva.hip — K4: funding valuation adjustment (funding cost, funding benefit and their difference) in one pass over the
// unsecured exposures.
//
// Per path, with c the counterparty, o the own name, x_k = dev_unsec at metric date k and the sums over k = 0 .. E-2:
//   w(k) = S_c(0,t_k) S_o(0,t_k)                      (a name without atoms never defaults: its S is 1)
//   fca  = sum relu( x_k) w(k) phi_b(k)               phi_b(k) = 1 - exp(-int_{t_k}^{t_k+1} s_b): the borrowing weight
//   fba  = sum relu(-x_k) w(k) phi_l(k)               phi_l(k): the lending weight
//   fva  = fca - fba                                  (per path: its Monte-Carlo error is that of the difference)
// The weights are deterministic: the host computes them in float64 (mcx/metrics/fva_metric.py funding_weights) and the call stages
// the two tables; the kernel reads them wave-uniformly (scalar loads), as it reads the atom ids.
//
// One launch, the shape of k4_xva: a lane owns a path (grid-stride over the paths), walks the dates once, reads x_k once per date,
// evaluates at most two atoms and keeps the three integrands in registers; the block reduction of the three shifted pairs
// (sum (v-c), sum (v-c)^2) follows in the same kernel.  The shift c is the integrand of the first local path: wave 0 of every block
// recomputes it (wave-uniform loads) and hands it to the other waves through LDS; no prologue launch.  No float atomics: one partial
// per block, then k_finish_acc (mcx_finish_acc) with 3 records, so the records are bitwise reproducible run to run.
//
// Operation order: w = Sc * So (commutative: swapping the names changes no byte), wb = w * phi_b, wl = w * phi_l, then one fma per
// leg; fva is the difference of the two finished legs in a statement of its own.  So swapping the weight tables and negating the
// exposures runs the SAME arithmetic on the other accumulator (fca <-> fba, fva -> -fva bit for bit), and with no names and unit
// weights every product is exact: fca is the sequential float64 sum of relu(x_k).
#include "mcx_internal.h"

namespace {

#define FVA_R 3

struct FvaArgs {
    DevUnsec u;
    const DevAtom* atoms;
    const int32_t* surv_c;    // device [n_dates-1] atom ids of S_c(0,t_k), or nullptr: the counterparty never defaults
    const int32_t* surv_o;    // the same for the own name
    const double* w_borrow;   // device [n_dates-1]
    const double* w_lend;
    const double* expo;
    const double* paths;
    int64_t D, n, ld_expo, ld_paths;
    double* partials;   // [grid][FVA_R][2]
    double* shifts;     // [FVA_R]
};

__device__ __forceinline__ void fva_path(const FvaArgs& a, int64_t i, double (&v)[FVA_R])
{
    double fca = 0.0, fba = 0.0;
    for (int m = 0; m < a.u.n_dates - 1; ++m) {
        const double x = dev_unsec(a.u, a.expo, a.ld_expo, m, i);
        const double ep = fmax(x, 0.0), en = fmax(-x, 0.0);
        double Sc = 1.0, So = 1.0;
        if (a.surv_c) Sc = dev_atom(ldk_struct(&a.atoms[ldk(a.surv_c + m)]), a.paths, a.D, a.ld_paths, i);   // wave-uniform tests
        if (a.surv_o) So = dev_atom(ldk_struct(&a.atoms[ldk(a.surv_o + m)]), a.paths, a.D, a.ld_paths, i);
        const double w = Sc * So;
        const double wb = w * ldk(a.w_borrow + m), wl = w * ldk(a.w_lend + m);
        fca = fma(ep, wb, fca);
        fba = fma(en, wl, fba);
    }
    v[0] = fca;
    v[1] = fba;
    v[2] = fca - fba;
}

__global__ __launch_bounds__(MCX_BLOCK) void k4_fva(const FvaArgs a)
{
    __shared__ double lds[FVA_R + 4 * 2 * FVA_R];
    if (threadIdx.x < MCX_WAVE) {                                   // the shifts: the integrands of path 0
        double c0[FVA_R];
        fva_path(a, 0, c0);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int r = 0; r < FVA_R; ++r) lds[r] = c0[r];
        }
    }
    __syncthreads();
    double c[FVA_R], s1[FVA_R], s2[FVA_R];
#pragma unroll
    for (int r = 0; r < FVA_R; ++r) { c[r] = lds[r]; s1[r] = 0.0; s2[r] = 0.0; }
    for (int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * MCX_BLOCK) {
        double v[FVA_R];
        fva_path(a, i, v);
#pragma unroll
        for (int r = 0; r < FVA_R; ++r) {
            const double d = v[r] - c[r];
            s1[r] += d; s2[r] = fma(d, d, s2[r]);
        }
    }
    // block sums: wave shuffles, then the 4 wave totals of every entry added in wave order by one thread per entry
    const int lane = threadIdx.x & (MCX_WAVE - 1), w = threadIdx.x >> 6;
    double* wsum = lds + FVA_R;                                     // [4 waves][FVA_R][2]
#pragma unroll
    for (int r = 0; r < FVA_R; ++r) {
        const double t1 = wave_sum(s1[r]), t2 = wave_sum(s2[r]);
        if (lane == 0) { wsum[(w * FVA_R + r) * 2 + 0] = t1; wsum[(w * FVA_R + r) * 2 + 1] = t2; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * FVA_R) {
        double t = 0.0;
        for (int q = 0; q < MCX_BLOCK / MCX_WAVE; ++q) t += wsum[q * 2 * FVA_R + threadIdx.x];
        a.partials[(int64_t)blockIdx.x * 2 * FVA_R + threadIdx.x] = t;
        if (blockIdx.x == 0 && threadIdx.x < FVA_R) a.shifts[threadIdx.x] = lds[threadIdx.x];
    }
}

}  // namespace

extern "C" int mcx_reduce_fva(mcx_handle* h, const mcx_book* b, const mcx_unsecured_desc* u,
                              const int32_t* h_surv_c, const int32_t* h_surv_o, const double* h_w_borrow, const double* h_w_lend,
                              const double* d_expo_ns, const double* d_paths, int64_t n_paths, int64_t ld_expo, int64_t ld_paths,
                              mcx_acc* h_out, void* stream)
{
    if (!h) return -1;
    if (!b || !u || !d_expo_ns || !d_paths || !h_w_borrow || !h_w_lend || !h_out)
        MCX_FAIL(h, -1, "mcx_reduce_fva: a NULL book, descriptor, buffer, weight table or h_out");
    if (n_paths <= 0) { memset(h_out, 0, sizeof(mcx_acc) * FVA_R); return 0; }
    if (ld_expo < n_paths || ld_paths < n_paths) MCX_FAIL(h, -2, "mcx_reduce_fva: leading dimension < n_paths");
    hipStream_t s = (hipStream_t)stream;
    DevUnsec du; int32_t* tmp = nullptr;
    int rc = mcx_upload_unsec(h, u, &du, &tmp, s);    // (checks n_dates first: the lists and tables below are read up to it)
    if (rc) return rc;
    const int nd = u->n_dates - 1;
    const int32_t* lists[2] = {h_surv_c, h_surv_o};
    for (int q = 0; q < 2; ++q)
        for (int m = 0; lists[q] && m < nd; ++m)
            if (lists[q][m] < 0 || lists[q][m] >= b->n_atoms) MCX_FAIL(h, -2, "mcx_reduce_fva: atom id out of range");
    for (int m = 0; m < u->n_dates; ++m)          // the rows index the netting set's exposure block of the book
        if (u->row[m] < 0 || u->row[m] >= b->n_expo_rows || (u->delayed && u->delayed[m] >= b->n_expo_rows))
            MCX_FAIL(h, -2, "mcx_reduce_fva: exposure row of metric date %d out of range", m);
    // one launch shape: up to 8 blocks per CU (every wave slot of the chip), the paths beyond that by the grid stride
    const int grid = mcx_grid_for(n_paths, MCX_BLOCK, 8 * h->n_cu);
    if (((size_t)grid * 2 + 1) * FVA_R * sizeof(double) > h->ws_bytes) MCX_FAIL(h, -2, "mcx_reduce_fva: workspace too small");
    FvaArgs a;
    a.u = du; a.atoms = b->d_atoms;
    a.surv_c = a.surv_o = nullptr;
    a.w_borrow = a.w_lend = nullptr;
    if (nd > 0) {
        std::vector<double> wts(h_w_borrow, h_w_borrow + nd);
        wts.insert(wts.end(), h_w_lend, h_w_lend + nd);
        const double* d_w = (const double*)mcx_stage_small(h, wts.data(), sizeof(double) * wts.size(), s);
        if (!d_w) return -100;
        a.w_borrow = d_w; a.w_lend = d_w + nd;
        if (h_surv_c || h_surv_o) {
            std::vector<int32_t> ids;
            for (int q = 0; q < 2; ++q)
                if (lists[q]) ids.insert(ids.end(), lists[q], lists[q] + nd);
            const int32_t* d_ids = (const int32_t*)mcx_stage_small(h, ids.data(), sizeof(int32_t) * ids.size(), s);
            if (!d_ids) return -100;
            if (h_surv_c) { a.surv_c = d_ids; d_ids += nd; }
            if (h_surv_o) a.surv_o = d_ids;
        }
    }
    a.expo = d_expo_ns; a.paths = d_paths;
    a.D = (int64_t)b->n_state; a.n = n_paths; a.ld_expo = ld_expo; a.ld_paths = ld_paths;
    a.partials = h->d_ws;
    a.shifts = h->d_ws + (size_t)grid * 2 * FVA_R;
    hipLaunchKernelGGL(k4_fva, dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    MCX_HIP(h, hipGetLastError());
    return mcx_finish_acc(h, a.partials, FVA_R, grid, (double)n_paths, a.shifts, h_out, s);
}
