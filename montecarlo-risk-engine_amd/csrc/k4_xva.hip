// k4_xva.hip — K4: bilateral xVA (CVA, DVA and their first-to-default forms) in one pass over the unsecured exposures.
//
// Per path, with c the counterparty, o the own name, x_k = dev_unsec at metric date k and the sums over k = 0 .. E-2:
//   cva     = (1-R_c) sum relu( x_k) S_c(k) q_c(k)            (cva_metric.py:88-99 of the reference, k4_cva_paths)
//   dva     = (1-R_o) sum relu(-x_k) S_o(k) q_o(k)
//   cva_ftd = (1-R_c) sum relu( x_k) S_c(k) q_c(k) S_o(k)
//   dva_ftd = (1-R_o) sum relu(-x_k) S_o(k) q_o(k) S_c(k)
//   bcva    = cva_ftd - dva_ftd                                (per path: its Monte-Carlo error is that of the difference)
// S_n(k) = S_n(0, t_k) and q_n(k) = 1 - S_n(t_k, t_{k+1}) are the two atoms per date CVAMetric registers, here for two names.
//
// One launch: a lane owns a path (grid-stride over the paths), walks the dates once, reads x_k once per date and keeps the five
// integrands in registers; the block reduction of the five shifted pairs (sum (v-c), sum (v-c)^2) follows in the same kernel —
// a second pass (k4_cva_paths -> k4_vector) would write and re-read five vectors.  The shift c is the integrand of the first local
// path: wave 0 of every block recomputes it (its loads at path 0 are wave-uniform, so they hit in cache) and hands it to the
// other waves through LDS; no prologue launch, no cross-block dependency.  No float atomics: one partial per block, then
// k_finish_acc (mcx_finish_acc) with 5 records, so the records are bitwise reproducible run to run.
//
// Operation order: every product is written so that swapping the two names and negating the exposures runs the SAME arithmetic
// on the other accumulator (cva <-> dva, cva_ftd <-> dva_ftd, bcva -> -bcva bit for bit): the weights are S q first, then times
// the other name's S; bcva is the difference of the two already scaled legs, formed in a statement of its own (no contraction).
#include "mcx_internal.h"

namespace {

#define XVA_R 5

// one party: atom ids of S(0,t_k) and S(t_k,t_{k+1}) per date (device, [n_dates-1]); surv == nullptr: it never defaults
struct XvaSide {
    const int32_t* surv;
    const int32_t* cond;
    double lgd;
};

struct XvaArgs {
    DevUnsec u;
    const DevAtom* atoms;
    XvaSide c, o;
    const double* expo;
    const double* paths;
    int64_t D, n, ld_expo, ld_paths;
    double* partials;   // [grid][XVA_R][2]
    double* shifts;     // [XVA_R]
};

__device__ __forceinline__ void xva_side(const DevAtom* __restrict__ atoms, const XvaSide& s, int m, const double* __restrict__ paths,
                                         int64_t D, int64_t ld, int64_t i, double& S, double& q)
{
    S = 1.0; q = 0.0;
    if (s.surv) {                                                   // wave-uniform
        S = dev_atom(ldk_struct(&atoms[ldk(s.surv + m)]), paths, D, ld, i);
        q = 1.0 - dev_atom(ldk_struct(&atoms[ldk(s.cond + m)]), paths, D, ld, i);
    }
}

__device__ __forceinline__ void xva_path(const XvaArgs& a, int64_t i, double (&v)[XVA_R])
{
    double cva = 0.0, dva = 0.0, cftd = 0.0, dftd = 0.0;
    for (int m = 0; m < a.u.n_dates - 1; ++m) {
        const double x = dev_unsec(a.u, a.expo, a.ld_expo, m, i);
        const double ep = fmax(x, 0.0), en = fmax(-x, 0.0);
        double Sc, qc, So, qo;
        xva_side(a.atoms, a.c, m, a.paths, a.D, a.ld_paths, i, Sc, qc);
        xva_side(a.atoms, a.o, m, a.paths, a.D, a.ld_paths, i, So, qo);
        const double wc = Sc * qc, wo = So * qo;
        const double wcf = wc * So, wof = wo * Sc;
        cva = fma(ep, wc, cva);
        dva = fma(en, wo, dva);
        cftd = fma(ep, wcf, cftd);
        dftd = fma(en, wof, dftd);
    }
    v[0] = cva * a.c.lgd;
    v[1] = dva * a.o.lgd;
    v[2] = cftd * a.c.lgd;
    v[3] = dftd * a.o.lgd;
    v[4] = v[2] - v[3];
}

__global__ __launch_bounds__(MCX_BLOCK) void k4_xva(const XvaArgs a)
{
    __shared__ double lds[XVA_R + 4 * 2 * XVA_R];
    if (threadIdx.x < MCX_WAVE) {                                   // the shifts: the integrands of path 0
        double c0[XVA_R];
        xva_path(a, 0, c0);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int r = 0; r < XVA_R; ++r) lds[r] = c0[r];
        }
    }
    __syncthreads();
    double c[XVA_R], s1[XVA_R], s2[XVA_R];
#pragma unroll
    for (int r = 0; r < XVA_R; ++r) { c[r] = lds[r]; s1[r] = 0.0; s2[r] = 0.0; }
    for (int64_t i = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * MCX_BLOCK) {
        double v[XVA_R];
        xva_path(a, i, v);
#pragma unroll
        for (int r = 0; r < XVA_R; ++r) {
            const double d = v[r] - c[r];
            s1[r] += d; s2[r] = fma(d, d, s2[r]);
        }
    }
    // block sums: wave shuffles, then the 4 wave totals of every entry added in wave order by one thread per entry
    const int lane = threadIdx.x & (MCX_WAVE - 1), w = threadIdx.x >> 6;
    double* wsum = lds + XVA_R;                                     // [4 waves][XVA_R][2]
#pragma unroll
    for (int r = 0; r < XVA_R; ++r) {
        const double t1 = wave_sum(s1[r]), t2 = wave_sum(s2[r]);
        if (lane == 0) { wsum[(w * XVA_R + r) * 2 + 0] = t1; wsum[(w * XVA_R + r) * 2 + 1] = t2; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * XVA_R) {
        double t = 0.0;
        for (int q = 0; q < MCX_BLOCK / MCX_WAVE; ++q) t += wsum[q * 2 * XVA_R + threadIdx.x];
        a.partials[(int64_t)blockIdx.x * 2 * XVA_R + threadIdx.x] = t;
        if (blockIdx.x == 0 && threadIdx.x < XVA_R) a.shifts[threadIdx.x] = lds[threadIdx.x];
    }
}

}  // namespace

extern "C" int mcx_reduce_xva(mcx_handle* h, const mcx_book* b, const mcx_unsecured_desc* u,
                              const int32_t* h_surv_c, const int32_t* h_cond_c, double recovery_c,
                              const int32_t* h_surv_o, const int32_t* h_cond_o, double recovery_o,
                              const double* d_expo_ns, const double* d_paths, int64_t n_paths, int64_t ld_expo, int64_t ld_paths,
                              mcx_acc* h_out, void* stream)
{
    if (!h || !b || !u || !d_expo_ns || !d_paths || !h_out) return -1;
    if (n_paths <= 0) { memset(h_out, 0, sizeof(mcx_acc) * XVA_R); return 0; }
    if (ld_expo < n_paths || ld_paths < n_paths) MCX_FAIL(h, -2, "mcx_reduce_xva: leading dimension < n_paths");
    if (!h_surv_c != !h_cond_c || !h_surv_o != !h_cond_o)
        MCX_FAIL(h, -2, "mcx_reduce_xva: the survival and conditional-survival atoms of a name come together (both or neither)");
    hipStream_t s = (hipStream_t)stream;
    DevUnsec du; int32_t* tmp = nullptr;
    int rc = mcx_upload_unsec(h, u, &du, &tmp, s);    // (checks n_dates first: the atom lists below are read up to it)
    if (rc) return rc;
    const int nd = u->n_dates - 1;
    const int32_t* lists[4] = {h_surv_c, h_cond_c, h_surv_o, h_cond_o};
    for (int q = 0; q < 4; ++q)
        for (int m = 0; lists[q] && m < nd; ++m)
            if (lists[q][m] < 0 || lists[q][m] >= b->n_atoms) MCX_FAIL(h, -2, "mcx_reduce_xva: atom id out of range");
    for (int m = 0; m < u->n_dates; ++m)          // the rows index the netting set's exposure block of the book
        if (u->row[m] < 0 || u->row[m] >= b->n_expo_rows || (u->delayed && u->delayed[m] >= b->n_expo_rows))
            MCX_FAIL(h, -2, "mcx_reduce_xva: exposure row of metric date %d out of range", m);
    XvaArgs a;
    a.u = du; a.atoms = b->d_atoms;
    a.c = {nullptr, nullptr, 1.0 - recovery_c};
    a.o = {nullptr, nullptr, 1.0 - recovery_o};
    if (nd > 0 && (h_surv_c || h_surv_o)) {
        std::vector<int32_t> ids;
        for (int q = 0; q < 4; ++q)
            if (lists[q]) ids.insert(ids.end(), lists[q], lists[q] + nd);
        const int32_t* d_ids = (const int32_t*)mcx_stage_small(h, ids.data(), sizeof(int32_t) * ids.size(), s);
        if (!d_ids) return -100;
        if (h_surv_c) { a.c.surv = d_ids; a.c.cond = d_ids + nd; d_ids += 2 * nd; }
        if (h_surv_o) { a.o.surv = d_ids; a.o.cond = d_ids + nd; }
    }
    a.expo = d_expo_ns; a.paths = d_paths;
    a.D = (int64_t)b->n_state; a.n = n_paths; a.ld_expo = ld_expo; a.ld_paths = ld_paths;
    // one launch shape: up to 8 blocks per CU (every wave slot of the chip), the paths beyond that by the grid stride
    const int grid = mcx_grid_for(n_paths, MCX_BLOCK, 8 * h->n_cu);
    if (((size_t)grid * 2 + 1) * XVA_R * sizeof(double) > h->ws_bytes) MCX_FAIL(h, -2, "mcx_reduce_xva: workspace too small");
    a.partials = h->d_ws;
    a.shifts = h->d_ws + (size_t)grid * 2 * XVA_R;
    hipLaunchKernelGGL(k4_xva, dim3(grid), dim3(MCX_BLOCK), 0, s, a);
    MCX_HIP(h, hipGetLastError());
    return mcx_finish_acc(h, a.partials, XVA_R, grid, (double)n_paths, a.shifts, h_out, s);
}
