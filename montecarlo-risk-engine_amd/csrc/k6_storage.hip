// k6_storage.hip — K6: the gas storage (products/storage.py of the reference; include/mcx.h "K6 — gas storage").
//
// The storage's Longstaff-Schwartz state is a real number s in [0, S-1] (position of the inventory in the volume window of the
// date), so neither the exercise machine of k3_lsm.hip (integer states, one decision bit) nor the event program of k2_book.hip
// fits.  The kernels:
//   k6_step          one backward date: every path rolls ALL S integer start states one action date forward (the next states and
//                    volume changes of integer states are path-independent: the host's transition table, scalar loads), writes
//                    W_new[s] = cash / numeraire + lerp(W_old, next state) and accumulates the moments of the regression.
//                    One path per lane; a moment is reduced over the wave as soon as it is formed (S*K of them do not fit in
//                    registers), lane 0 of each wave adds it to the wave's LDS row, one barrier at the end.
//   k6_finish_solve  sums the per-block partials and solves the K x K normal equations for S right-hand sides, lane s taking
//                    state s (lsm_solve.h, the solver k3_lsm.hip calls too: LU with partial pivoting, back-transformation of the
//                    shifted / scaled basis, minimum-norm solution of the exactly rank-1 system of the calibration date).
//   k6_step_batch / k6_finish_solve_batch   the same two for step r of MANY storages in one launch each (grid.y resp. grid.x = job):
//                    the bodies of k6_step / k6_finish_solve as device functions, the job's record read with scalar loads.
//   k6_eval          main simulation: the realised state of a path in a register, walked through the action dates and the
//                    exposure rows; the date record and its [S][K] coefficient block are staged in LDS once per block and date.
// Exact ties between candidates are the rule (a full store: inject == hold): every candidate goes through ONE inline function,
// so tied candidates are bit-identical, and the first of [inject, hold, withdraw] wins as torch.argmax does.
// The per-path arithmetic up to the candidates, the date record and its host checks live in k6_common.h, which kt_storage.hip
// (the tangent images of k6_step and k6_eval) shares.
#include "k6_common.h"
#include "lsm_solve.h"

#include <stdlib.h>

#include <algorithm>

struct mcx_storage {
    int n_states, n_dates, netting_set, n_basis;
    int64_t n_coeffs;           // of the book the storage was created on
    K6Date* d_dates;
    double* d_trans;            // [n_dates][S][3][2]
    std::vector<K6Date> h_dates;
};

namespace {

// ---- backward step ---------------------------------------------------------------------------------------------------
struct K6StepArgs {                        // kernel argument of k6_step; one record of k6_step_batch's job table
    const double* __restrict__ paths;
    const double* __restrict__ W_old;
    double* __restrict__ W_new;
    double* __restrict__ partials;         // [gridDim.x][NM]
    const double* __restrict__ coeffs;     // [S][K] block of the rolled date (unused when is_last)
    const double* __restrict__ trans;      // [S][3][2] of the rolled date
    DevAtom num, x;                        // regression date
    DevAtom rnum, rx;                      // rolled action date
    double shift, scale, c_inj, c_wd;
    int64_t n, ld, ld_w;
    int32_t S, n_state, roll, is_last, f32_cache;
};
static_assert(sizeof(K6StepArgs) % 4 == 0, "read with ldk_struct");

// the backward step of ONE storage for the block's tiles (blockIdx.x of gridDim.x): shared by k6_step and k6_step_batch, so the
// per-path arithmetic, the wave_sum order and the FMA contraction of the two kernels are the same program text
template <int K>
__device__ __forceinline__ void k6_step_body(const K6StepArgs a)          // (by value: k6_step then compiles to the code it had as a kernel of its own)
{
    constexpr int NB = 2 * K - 1;
    __shared__ double rows[4][NB + K6_MAX_S * K];
    const int NM = NB + a.S * K;
    const int lane = threadIdx.x & (MCX_WAVE - 1), wv = threadIdx.x >> 6;
    for (int q = lane; q < NM; q += MCX_WAVE) rows[wv][q] = 0.0;       // (each wave owns its row: no barrier needed before use)
    const int64_t D = a.n_state;
    for (int64_t base = (int64_t)blockIdx.x * MCX_BLOCK; base < a.n; base += (int64_t)gridDim.x * MCX_BLOCK) {
        const int64_t i_raw = base + threadIdx.x;
        const bool live = i_raw < a.n;
        const int64_t i = live ? i_raw : a.n - 1;                       // idle lanes read a valid path and contribute zero
        const double num = dev_atom(a.num, a.paths, D, a.ld, i);
        const double z = (dev_atom(a.x, a.paths, D, a.ld, i) - a.shift) * a.scale;
        double zp = 1.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const double r = wave_sum(live ? zp : 0.0);
            if (lane == 0) rows[wv][k] += r;
            zp *= z;
        }
        double spot = 0.0, rnum = 1.0;
        if (a.roll) { spot = dev_atom(a.rx, a.paths, D, a.ld, i); rnum = dev_atom(a.rnum, a.paths, D, a.ld, i); }
        const double p_inj = spot + a.c_inj, p_wd = spot - a.c_wd;
        for (int s = 0; s < a.S; ++s) {
            double w;
            if (a.roll) {
                const double* __restrict__ t = a.trans + s * 6;
                const double ns0 = ldk(t + 0), dv0 = ldk(t + 1), ns1 = ldk(t + 2), dv1 = ldk(t + 3), ns2 = ldk(t + 4), dv2 = ldk(t + 5);
                double c0, v0, t0, c1, v1, t1, c2, v2, t2, f;
                int lo, hi;                                                // (where the tail was read: the tangent kernel's)
                k6_step_candidate<K>(a.coeffs, a.W_old, a.ld_w, a.S, a.is_last, ns0, dv0, p_inj, spot, i, c0, v0, t0, lo, hi, f);                      // inject
                k6_step_candidate<K>(a.coeffs, a.W_old, a.ld_w, a.S, a.is_last, ns1, dv1, dv1 >= 0.0 ? p_inj : p_wd, spot, i, c1, v1, t1, lo, hi, f);  // hold
                k6_step_candidate<K>(a.coeffs, a.W_old, a.ld_w, a.S, a.is_last, ns2, dv2, p_wd, spot, i, c2, v2, t2, lo, hi, f);                      // withdraw
                double cb = c0, vb = v0, tb = t0;                          // the first maximum wins (torch.argmax)
                if (v1 > vb) { cb = c1; vb = v1; tb = t1; }
                if (v2 > vb) { cb = c2; vb = v2; tb = t2; }
                double c = cb / rnum;
                if (a.f32_cache) c = (double)(float)c;                     // float32 step buffer (controller.py:330, 341)
                w = c + tb;
                if (live) a.W_new[(int64_t)s * a.ld_w + i] = w;
            } else {
                w = a.W_old[(int64_t)s * a.ld_w + i];
            }
            const double y = num * w;
            zp = 1.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double r = wave_sum(live ? zp * y : 0.0);
                if (lane == 0) rows[wv][NB + s * K + k] += r;
                zp *= z;
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < NM; q += MCX_BLOCK)
        a.partials[(int64_t)blockIdx.x * NM + q] = (rows[0][q] + rows[1][q]) + (rows[2][q] + rows[3][q]);
}

template <int K>
__global__ __launch_bounds__(MCX_BLOCK) void k6_step(const K6StepArgs a)
{
    k6_step_body<K>(a);
}

// step r of MANY storages in one launch: grid (tiles, jobs), blockIdx.y selects the job.  Its record is a complete K6StepArgs
// (block-uniform: scalar loads) whose `partials` points at the job's own [tiles][NM_j] block, so every block does for its job
// exactly what a k6_step block does for its single storage.  Jobs of one launch share paths and path count (the same tiling);
// S, the roll and the atoms differ per job.
template <int K>
__global__ __launch_bounds__(MCX_BLOCK) void k6_step_batch(const K6StepArgs* __restrict__ jobs)
{
    const K6StepArgs a = ldk_struct(jobs + blockIdx.y);
    k6_step_body<K>(a);
}

// ---- solve -----------------------------------------------------------------------------------------------------------
struct K6Solve {
    double shift, scale, x0;
    int64_t off0, off1;
    int32_t degenerate, S, date, pad;
};

// right-hand side s of the K x K system in m[]: lsm_solve (lsm_solve.h) for one state, every lane factorises the same Gram matrix in
// registers; here only the stores.  table: the system's own [S][K] block or nullptr, status: the system's own word
template <int K>
__device__ __forceinline__ void k6_solve_state(const double* __restrict__ m, const K6Solve& q, int s, double* __restrict__ coeffs,
                                               double* __restrict__ table, int32_t* __restrict__ status)
{
    double out[1][K];
    const int st = lsm_solve<K, 1>(m, K, s, 1, q.shift, q.scale, q.x0, q.degenerate, out);
    if (s == 0) *status = st;                                          // numerically singular: reported, not written
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (table) table[s * K + k] = out[0][k];
        if (st == 0) {
            if (q.off0 >= 0) coeffs[q.off0 + s * K + k] = out[0][k];
            if (q.off1 >= 0) coeffs[q.off1 + s * K + k] = out[0][k];
        }
    }
}

// n_blocks > 0: wave q of the block sums moment q over the step kernel's partials (fixed order) into LDS and mom_out, and zeroes
// mom_out[nm .. mom_len) (the padding of a batched step's row; mom_len <= nm: none);
// n_blocks == 0: the moments are read from mom_out (all-reduced by the caller).  do_solve: lane s < S then solves state s.
template <int K>
__device__ __forceinline__ void k6_finish_body(const double* __restrict__ partials, int n_blocks, double* __restrict__ mom_out, int mom_len,
                                               int do_solve, const K6Solve& q, double* __restrict__ coeffs, double* __restrict__ table,
                                               int32_t* __restrict__ status)
{
    __shared__ double m[(2 * K - 1) + K6_MAX_S * K];
    const int nm = (2 * K - 1) + q.S * K;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (n_blocks > 0) {
        for (int j = wv; j < nm; j += 16) {
            double s = 0.0;
            for (int b = lane; b < n_blocks; b += MCX_WAVE) s += partials[(int64_t)b * nm + j];
            s = wave_sum(s);
            if (lane == 0) { m[j] = s; mom_out[j] = s; }
        }
        for (int j = nm + threadIdx.x; j < mom_len; j += 1024) mom_out[j] = 0.0;
    } else {
        for (int j = threadIdx.x; j < nm; j += 1024) m[j] = mom_out[j];
    }
    __syncthreads();
    if (do_solve && (int)threadIdx.x < q.S) k6_solve_state<K>(m, q, threadIdx.x, coeffs, table, status);
}

// one storage: table [n_dates][S][K] and status [n_dates] of the run, the system is date q.date
template <int K>
__global__ __launch_bounds__(1024) void k6_finish_solve(const double* __restrict__ partials, int n_blocks, double* __restrict__ mom_out,
                                                        int do_solve, const K6Solve q, double* __restrict__ coeffs,
                                                        double* __restrict__ table, int32_t* __restrict__ status)
{
    k6_finish_body<K>(partials, n_blocks, mom_out, 0, do_solve, q, coeffs, table ? table + (int64_t)q.date * q.S * K : nullptr,
                      status + q.date);
}

// one block per job of a batched step (the record is block-uniform: scalar loads).  Row blockIdx.x of `mom` ([jobs][mom_stride],
// zero-padded behind the job's NM moments, so ONE all-reduce covers the step); the job's [S][K] block of the packed table at
// tab_off; status[q.date], q.date = the job's index in the table of the call.  do_sum == 0: the moments are read (all-reduced).
struct K6BatchSolve {
    K6Solve q;
    int64_t part_off, tab_off;          // doubles: the job's [n_blocks][NM] partials in the launch's buffer; its block of the table
    int32_t n_blocks, pad;
};
static_assert(sizeof(K6BatchSolve) % 8 == 0, "read with ldk_struct");

template <int K>
__global__ __launch_bounds__(1024) void k6_finish_solve_batch(const K6BatchSolve* __restrict__ jobs, const double* __restrict__ partials,
                                                              int do_sum, double* __restrict__ mom, int64_t mom_stride, int do_solve,
                                                              double* __restrict__ coeffs, double* __restrict__ table,
                                                              int32_t* __restrict__ status)
{
    const K6BatchSolve j = ldk_struct(jobs + blockIdx.x);
    k6_finish_body<K>(partials + j.part_off, do_sum ? j.n_blocks : 0, mom + (int64_t)blockIdx.x * mom_stride, (int)mom_stride, do_solve,
                      j.q, coeffs, table ? table + j.tab_off : nullptr, status + j.q.date);
}

// ---- main simulation -------------------------------------------------------------------------------------------------
struct K6EvalArgs {
    const double* __restrict__ paths;
    const K6Date* __restrict__ dates;
    const mcx_storage_op* __restrict__ ops;
    const DevAtom* __restrict__ atoms;
    const double* __restrict__ coeffs;
    double* __restrict__ cfs;              // the netting set's row or nullptr
    double* __restrict__ expo;             // the netting set's [n_expo_rows][ld_out] block or nullptr
    int64_t n, ld, ld_out;
    int32_t n_ops, S, n_state, pad;
};

template <int K>
__global__ __launch_bounds__(MCX_BLOCK) void k6_eval(const K6EvalArgs a)
{
    __shared__ K6Date sd;
    __shared__ double sc[K6_MAX_S * K];
    const int64_t i_raw = (int64_t)blockIdx.x * MCX_BLOCK + threadIdx.x;
    const bool live = i_raw < a.n;
    const int64_t i = live ? i_raw : a.n - 1;
    const int64_t D = a.n_state;
    double state = 0.0, cf = 0.0;                                       // get_initial_state() = 0.0
    for (int op = 0; op < a.n_ops; ++op) {
        const mcx_storage_op o = ldk_struct(a.ops + op);
        __syncthreads();                                                // the previous op's readers are done with sd / sc
        int64_t off = o.coeff_off;
        bool need_coeffs = true;
        if (o.kind == 0) {
            const uint32_t* __restrict__ src = (const uint32_t*)(a.dates + o.index);
            for (int q = threadIdx.x; q < (int)(sizeof(K6Date) / 4); q += MCX_BLOCK) ((uint32_t*)&sd)[q] = src[q];
            off = ldk(&a.dates[o.index].coeff_off);
            need_coeffs = ldk(&a.dates[o.index].is_last) == 0;
        }
        if (need_coeffs)
            for (int q = threadIdx.x; q < a.S * K; q += MCX_BLOCK) sc[q] = a.coeffs[off + q];
        __syncthreads();
        if (o.kind == 0) {
            const double spot = dev_atom(sd.x, a.paths, D, a.ld, i), num = dev_atom(sd.num, a.paths, D, a.ld, i);
            K6Cand c0, c1, c2;                                          // inject, hold, withdraw
            k6_eval_candidates<K>(sd, sc, a.S, state, spot, c0, c1, c2);
            double sb = c0.ns, cb = c0.cash, vb = c0.value;             // the first maximum wins (torch.argmax)
            if (c1.value > vb) { sb = c1.ns; cb = c1.cash; vb = c1.value; }
            if (c2.value > vb) { sb = c2.ns; cb = c2.cash; vb = c2.value; }
            state = sb;
            cf += cb / num;
        } else {
            const DevAtom an = ldk_struct(a.atoms + o.num_atom), ax = ldk_struct(a.atoms + o.x_atom);
            const double x = dev_atom(ax, a.paths, D, a.ld, i), num = dev_atom(an, a.paths, D, a.ld, i);
            const double e = k6_lerp_grid<K>(sc, a.S, state, x) / num;
            if (live && a.expo) a.expo[(int64_t)o.index * a.ld_out + i] += e;
        }
    }
    if (live && a.cfs) a.cfs[i] += cf;
}

// the K6StepArgs of one (storage, date) pair, `partials` left to the caller.  roll_date < 0: no roll (W_new unused)
K6StepArgs k6_fill_step(const mcx_book* b, const mcx_storage* st, int32_t roll_date, int32_t num_atom, int32_t x_atom, double shift,
                        double scale, const double* d_paths, int64_t n_paths, int64_t ld, const double* d_W_old, double* d_W_new,
                        int64_t ld_w, int32_t flags)
{
    K6StepArgs a;
    memset(&a, 0, sizeof(a));
    const int S = st->n_states;
    a.paths = d_paths; a.W_old = d_W_old; a.W_new = d_W_new;
    a.num = mcx_flat_atom(b->h_atoms[num_atom]); a.x = mcx_flat_atom(b->h_atoms[x_atom]);
    a.shift = shift; a.scale = scale; a.n = n_paths; a.ld = ld; a.ld_w = ld_w; a.S = S; a.n_state = b->n_state;
    a.f32_cache = (flags & MCX_LSM_F32_CACHE) ? 1 : 0;
    a.roll = roll_date >= 0;
    a.coeffs = b->d_coeffs; a.trans = st->d_trans; a.rnum = a.num; a.rx = a.x; a.c_inj = a.c_wd = 0.0; a.is_last = 1;
    if (a.roll) {
        const K6Date& d = st->h_dates[roll_date];
        a.coeffs = b->d_coeffs + d.coeff_off; a.trans = st->d_trans + (size_t)roll_date * S * 6;
        a.rnum = d.num; a.rx = d.x; a.c_inj = d.c_inj; a.c_wd = d.c_wd; a.is_last = d.is_last;
    }
    return a;
}

// the K6Solve of a date of mcx_storage_lsm_run or of a job (the two records name these fields alike); date: index of its status word
template <class Q>
K6Solve k6_fill_solve(const Q& q, int S, int date)
{
    K6Solve v;
    memset(&v, 0, sizeof(v));
    v.shift = q.shift; v.scale = q.scale; v.x0 = q.x0; v.off0 = q.coeff_off[0]; v.off1 = q.coeff_off[1];
    v.degenerate = q.degenerate; v.S = S; v.date = date;
    return v;
}

// step of one date on the stream: per-block partials in h->d_ws, *grid_out blocks (0: no paths)
int k6_step_launch(mcx_handle* h, const mcx_book* b, const mcx_storage* st, int32_t roll_date, int32_t num_atom, int32_t x_atom,
                   double shift, double scale, const double* d_paths, int64_t n_paths, int64_t ld, const double* d_W_old,
                   double* d_W_new, int64_t ld_w, int32_t flags, hipStream_t s, const char* who, int* grid_out)
{
    if (st->n_basis != b->n_basis || st->n_coeffs != b->n_coeffs) MCX_FAIL(h, -2, "%s: the storage was created on another book", who);
    if (roll_date >= st->n_dates) MCX_FAIL(h, -2, "%s: roll date out of range", who);
    if (num_atom < 0 || num_atom >= b->n_atoms || x_atom < 0 || x_atom >= b->n_atoms) MCX_FAIL(h, -2, "%s: atom out of range", who);
    if (ld < n_paths || ld_w < n_paths) MCX_FAIL(h, -2, "%s: leading dimension < n_paths", who);
    if (roll_date >= 0 && (!d_W_new || d_W_new == d_W_old)) MCX_FAIL(h, -2, "%s: a roll needs a second cache buffer", who);
    const int K = st->n_basis, S = st->n_states, NM = (2 * K - 1) + S * K;
    *grid_out = 0;
    if (n_paths <= 0) return 0;
    const int grid = mcx_grid_for(n_paths, MCX_BLOCK, 4 * h->n_cu);
    if ((size_t)grid * NM * sizeof(double) > h->ws_bytes) MCX_FAIL(h, -2, "%s: workspace too small", who);
    K6StepArgs a = k6_fill_step(b, st, roll_date, num_atom, x_atom, shift, scale, d_paths, n_paths, ld, d_W_old, d_W_new, ld_w, flags);
    a.partials = h->d_ws;
    K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_step<KK>), dim3(grid), dim3(MCX_BLOCK), 0, s, a));
    MCX_HIP(h, hipGetLastError());
    *grid_out = grid;
    return 0;
}

}  // namespace

extern "C" int mcx_storage_create(mcx_handle* h, const mcx_book* b, const mcx_storage_desc* d, mcx_storage** out)
{
    if (!h || !b || !d || !out) return -1;
    if (int rc = k6_check_desc(h, b, d, "mcx_storage_create")) return rc;
    const int S = d->n_states, K = b->n_basis;
    std::vector<K6Date> dates((size_t)d->n_dates);
    for (int j = 0; j < d->n_dates; ++j) {
        if (int rc = k6_check_date(h, b, d, j, "mcx_storage_create")) return rc;
        k6_fill_date(b, d->dates[j], dates[j]);
    }
    MCX_HIP(h, hipSetDevice(h->device));
    mcx_storage* st = new mcx_storage();
    st->n_states = S; st->n_dates = d->n_dates; st->netting_set = d->netting_set; st->n_basis = K; st->n_coeffs = b->n_coeffs;
    st->d_dates = nullptr; st->d_trans = nullptr;
    st->h_dates = dates;
    const size_t db = sizeof(K6Date) * dates.size(), tb = sizeof(double) * (size_t)d->n_dates * S * 6;
    if (hipMalloc((void**)&st->d_dates, db) != hipSuccess || hipMalloc((void**)&st->d_trans, tb) != hipSuccess ||
        hipMemcpy(st->d_dates, dates.data(), db, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(st->d_trans, d->trans, tb, hipMemcpyHostToDevice) != hipSuccess) {
        mcx_storage_destroy(st);
        MCX_FAIL(h, -100, "mcx_storage_create: device allocation / upload failed");
    }
    *out = st;
    return 0;
}

extern "C" void mcx_storage_destroy(mcx_storage* st)
{
    if (!st) return;
    hipFree(st->d_dates);
    hipFree(st->d_trans);
    delete st;
}

extern "C" int mcx_storage_lsm_step(mcx_handle* h, const mcx_book* b, const mcx_storage* st, int32_t roll_date, int32_t num_atom,
                                    int32_t x_atom, double shift, double scale, const double* d_paths, int64_t n_paths, int64_t ld,
                                    const double* d_W_old, double* d_W_new, int64_t ld_w, double* d_moments, int32_t flags, void* stream)
{
    if (!h || !b || !st || !d_paths || !d_W_old || !d_moments) return -1;
    hipStream_t s = (hipStream_t)stream;
    const int K = st->n_basis, NM = (2 * K - 1) + st->n_states * K;
    int grid = 0;
    const int rc = k6_step_launch(h, b, st, roll_date, num_atom, x_atom, shift, scale, d_paths, n_paths, ld, d_W_old, d_W_new, ld_w,
                                  flags, s, "mcx_storage_lsm_step", &grid);
    if (rc != 0) return rc;
    if (grid == 0) { MCX_HIP(h, hipMemsetAsync(d_moments, 0, sizeof(double) * NM, s)); return 0; }
    K6Solve sv;
    memset(&sv, 0, sizeof(sv));
    sv.S = st->n_states;
    K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_finish_solve<KK>), dim3(1), dim3(1024), 0, s, h->d_ws, grid, d_moments, 0, sv,
                                      (double*)nullptr, (double*)nullptr, (int32_t*)nullptr));
    MCX_HIP(h, hipGetLastError());
    return 0;
}

extern "C" int mcx_storage_lsm_run(mcx_handle* h, mcx_book* b, const mcx_storage* st, const mcx_storage_lsm_date* h_dates, int32_t n_dates,
                                   const double* d_paths, int64_t n_paths, int64_t ld, double* d_W, int64_t ld_w,
                                   double* h_coeffs, int32_t* h_status, int32_t flags, void* stream)
{
    if (!h || !b || !st || !h_dates || !d_paths || !d_W || !h_coeffs || !h_status) return -1;
    if (n_dates <= 0) return 0;
    const int K = st->n_basis, S = st->n_states, NM = (2 * K - 1) + S * K;
    for (int d = 0; d < n_dates; ++d)
        for (int w = 0; w < 2; ++w)
            if (h_dates[d].coeff_off[w] >= 0 && h_dates[d].coeff_off[w] + (int64_t)S * K > b->n_coeffs)
                MCX_FAIL(h, -2, "mcx_storage_lsm_run: date %d coefficient offset out of range", d);
    const size_t tab_bytes = sizeof(double) * (size_t)n_dates * S * K, st_bytes = sizeof(int32_t) * (size_t)n_dates;
    hipStream_t s = (hipStream_t)stream;
    double* d_ws = (double*)mcx_scratch(h, 1, sizeof(double) * NM + tab_bytes + st_bytes + 64);
    if (!d_ws) return -100;
    double* d_mom = d_ws;
    double* d_tab = d_ws + NM;
    int32_t* d_st = (int32_t*)(d_tab + (size_t)n_dates * S * K);
    const bool multi = h->comm && h->comm_ranks > 1;
    int cur = 0, rc = 0;
    for (int d = 0; d < n_dates && rc == 0; ++d) {
        const mcx_storage_lsm_date& q = h_dates[d];
        double* W_old = d_W + (size_t)cur * S * ld_w;
        double* W_new = d_W + (size_t)(1 - cur) * S * ld_w;
        int grid = 0;
        rc = k6_step_launch(h, b, st, q.roll_date, q.num_atom, q.x_atom, q.shift, q.scale, d_paths, n_paths, ld, W_old, W_new, ld_w,
                            flags, s, "mcx_storage_lsm_run", &grid);
        if (rc != 0) break;
        if (q.roll_date >= 0) cur = 1 - cur;
        const K6Solve sv = k6_fill_solve(q, S, d);
        if (grid == 0 && hipMemsetAsync(d_mom, 0, sizeof(double) * NM, s) != hipSuccess) { h->err = "mcx_storage_lsm_run: memset failed"; rc = -100; break; }
        if (multi || grid == 0) {
            if (grid > 0) K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_finish_solve<KK>), dim3(1), dim3(1024), 0, s, h->d_ws, grid, d_mom, 0, sv,
                                                           b->d_coeffs, d_tab, d_st));
            if (multi) { rc = mcx_allreduce_f64(h, d_mom, NM, stream); if (rc != 0) break; }     // stream-ordered
            K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_finish_solve<KK>), dim3(1), dim3(1024), 0, s, (const double*)nullptr, 0, d_mom, 1, sv,
                                              b->d_coeffs, d_tab, d_st));
        } else {
            K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_finish_solve<KK>), dim3(1), dim3(1024), 0, s, h->d_ws, grid, d_mom, 1, sv,
                                              b->d_coeffs, d_tab, d_st));
        }
        if (hipGetLastError() != hipSuccess) { h->err = "mcx_storage_lsm_run: launch failed"; rc = -100; }
    }
    if (rc == 0 && (hipMemcpyAsync(h_coeffs, d_tab, tab_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipMemcpyAsync(h_status, d_st, st_bytes, hipMemcpyDeviceToHost, s) != hipSuccess)) { h->err = "mcx_storage_lsm_run: copy failed"; rc = -100; }
    if (hipStreamSynchronize(s) != hipSuccess && rc == 0) { h->err = "mcx_storage_lsm_run: synchronise failed"; rc = -100; }
    return rc;
}

// ---- product-batched backward induction ---------------------------------------------------------------------------------------
namespace {

// upper bound (bytes) of the partial sums one k6_step_batch launch may need: a step whose jobs need more is split over several
// launches, the tiling of a job never shrinks (a launch always takes at least one job: <= 4 n_cu tiles x 203 moments).
// MCX_STORAGE_BATCH_PARTIAL_BYTES overrides it (include/mcx.h); unset or unparsable: 64 MiB.
size_t k6_partial_cap()
{
    const char* e = getenv("MCX_STORAGE_BATCH_PARTIAL_BYTES");
    if (e && *e) {
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end != e && *end == 0 && v > 0) return (size_t)v;
    }
    return (size_t)64 << 20;
}
constexpr int K6_MAX_LAUNCH_JOBS = 32768;     // gridDim.y

struct K6Batch {
    std::vector<K6StepArgs> step;          // partials: set by k6_batch_place once the launch buffer is known
    std::vector<K6BatchSolve> solve;
    std::vector<int32_t> launch_begin;     // launches [launch_begin[l], launch_begin[l+1]) never cross a step
    size_t part_doubles = 0;               // of the largest launch
    int64_t tab_doubles = 0;               // of the packed coefficient table
    int widest = 0, nm_max = 0, tiles = 0; // jobs of the widest step; largest moment count; tiles per job
};

// what every batched entry point checks of job j before it reads the job's storage: the storage index, same book, at most once
// per step, coefficient offsets.  seen: [n_storages], the step each storage was last seen in (-2 at the start); step: of the job
// in the caller's table, -1 where the call is one step (which it cannot number)
int k6_check_job(mcx_handle* h, const mcx_book* b, const mcx_storage* const* storages, int32_t n_storages, const mcx_storage_lsm_job& q,
                 int j, int step, std::vector<int32_t>& seen, const char* who)
{
    if (q.storage < 0 || q.storage >= n_storages || !storages[q.storage]) MCX_FAIL(h, -2, "%s: job %d: storage index out of range", who, j);
    const mcx_storage* st = storages[q.storage];
    if (st->n_basis != b->n_basis || st->n_coeffs != b->n_coeffs) MCX_FAIL(h, -2, "%s: storage %d was created on another book", who, q.storage);
    if (seen[q.storage] == step) {
        if (step < 0) MCX_FAIL(h, -2, "%s: job %d: storage %d appears twice in the step", who, j, q.storage);
        MCX_FAIL(h, -2, "%s: job %d: storage %d appears twice in step %d", who, j, q.storage, step);
    }
    seen[q.storage] = step;
    for (int w = 0; w < 2; ++w)
        if (q.coeff_off[w] >= 0 && q.coeff_off[w] + (int64_t)st->n_states * b->n_basis > b->n_coeffs)
            MCX_FAIL(h, -2, "%s: job %d: coefficient offset out of range", who, j);
    return 0;
}

// every host-side check of a job table (nothing is launched before all of them pass) and its device image
int k6_batch_build(mcx_handle* h, const mcx_book* b, const mcx_storage* const* storages, int32_t n_storages,
                   const mcx_storage_lsm_job* h_jobs, const int32_t* h_step_begin, int32_t n_steps, const double* d_paths,
                   int64_t n_paths, int64_t ld, double* d_W, int64_t ld_w, int64_t w_len, int32_t flags, const char* who, K6Batch& out)
{
    const int K = b->n_basis;
    if (K < 1 || K > 6) MCX_FAIL(h, -3, "%s: unsupported basis size %d", who, K);
    if (n_storages < 1) MCX_FAIL(h, -2, "%s: no storages", who);
    if (ld < n_paths || ld_w < n_paths) MCX_FAIL(h, -2, "%s: leading dimension < n_paths", who);
    if (h_step_begin[0] != 0) MCX_FAIL(h, -2, "%s: step table must start at job 0", who);
    for (int q = 0; q < n_storages; ++q) {
        if (!storages[q]) MCX_FAIL(h, -2, "%s: storage %d is null", who, q);
        if (storages[q]->n_basis != K || storages[q]->n_coeffs != b->n_coeffs) MCX_FAIL(h, -2, "%s: storage %d was created on another book", who, q);
    }
    for (int t = 0; t < n_steps; ++t)
        if (h_step_begin[t + 1] < h_step_begin[t]) MCX_FAIL(h, -2, "%s: step table not ascending at step %d", who, t);
    const int n_jobs = h_step_begin[n_steps];
    out.tiles = n_paths > 0 ? mcx_grid_for(n_paths, MCX_BLOCK, 4 * h->n_cu) : 0;
    const size_t cap = k6_partial_cap() / sizeof(double);
    out.step.resize((size_t)n_jobs); out.solve.resize((size_t)n_jobs);
    out.launch_begin.assign(1, 0);
    std::vector<int32_t> seen((size_t)n_storages, -2);
    for (int t = 0; t < n_steps; ++t) {
        size_t used = 0;
        if (h_step_begin[t + 1] - h_step_begin[t] > out.widest) out.widest = h_step_begin[t + 1] - h_step_begin[t];
        for (int j = h_step_begin[t]; j < h_step_begin[t + 1]; ++j) {
            const mcx_storage_lsm_job& q = h_jobs[j];
            if (int rc = k6_check_job(h, b, storages, n_storages, q, j, t, seen, who)) return rc;
            const mcx_storage* st = storages[q.storage];
            const int S = st->n_states, NM = (2 * K - 1) + S * K;
            const bool roll = q.roll_date >= 0;
            if (q.roll_date >= st->n_dates) MCX_FAIL(h, -2, "%s: job %d: roll date out of range", who, j);
            if (q.num_atom < 0 || q.num_atom >= b->n_atoms || q.x_atom < 0 || q.x_atom >= b->n_atoms) MCX_FAIL(h, -2, "%s: job %d: atom out of range", who, j);
            const int64_t w_last = w_len - (int64_t)S * ld_w;
            if (q.w_old < 0 || q.w_old > w_last) MCX_FAIL(h, -2, "%s: job %d: w_old outside d_W", who, j);
            if (roll && (q.w_new < 0 || q.w_new > w_last)) MCX_FAIL(h, -2, "%s: job %d: w_new outside d_W", who, j);
            if (roll && q.w_new == q.w_old) MCX_FAIL(h, -2, "%s: job %d: a roll needs a second cache block (w_new == w_old)", who, j);
            // a new launch where the partials would pass the cap (or gridDim.y its limit); a launch holds at least one job
            const size_t need = (size_t)out.tiles * NM;
            if (j > out.launch_begin.back() && (used + need > cap || j - out.launch_begin.back() >= K6_MAX_LAUNCH_JOBS)) { out.launch_begin.push_back(j); used = 0; }
            out.step[j] = k6_fill_step(b, st, q.roll_date, q.num_atom, q.x_atom, q.shift, q.scale, d_paths, n_paths, ld, d_W + q.w_old,
                                       roll ? d_W + q.w_new : nullptr, ld_w, flags);
            K6BatchSolve& v = out.solve[j];
            memset(&v, 0, sizeof(v));
            v.q = k6_fill_solve(q, S, j);
            v.part_off = (int64_t)used; v.tab_off = out.tab_doubles; v.n_blocks = out.tiles;
            used += need;
            out.tab_doubles += (int64_t)S * K;
            if (used > out.part_doubles) out.part_doubles = used;
            if (NM > out.nm_max) out.nm_max = NM;
        }
        if (h_step_begin[t + 1] > out.launch_begin.back()) out.launch_begin.push_back(h_step_begin[t + 1]);
    }
    return 0;
}

void k6_batch_place(K6Batch& bt, double* d_part)
{
    for (size_t j = 0; j < bt.step.size(); ++j) bt.step[j].partials = d_part + bt.solve[j].part_off;
}

// the launches of jobs [j0, j1) of ONE step on the stream: k6_step_batch, then the fixed-order sums into rows j - j0 of d_mom
// (with the solve when do_solve).  n_paths <= 0: the rows are zeroed.
int k6_batch_step(mcx_handle* h, const mcx_book* b, const K6Batch& bt, const K6StepArgs* d_step, const K6BatchSolve* d_solve, int j0, int j1,
                  const double* d_part, double* d_mom, int64_t mom_stride, int do_solve, double* d_tab, int32_t* d_st, hipStream_t s)
{
    const int K = b->n_basis;
    if (j1 <= j0) return 0;
    if (bt.tiles == 0) {
        MCX_HIP(h, hipMemsetAsync(d_mom, 0, sizeof(double) * (size_t)(j1 - j0) * mom_stride, s));
        if (do_solve) K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_finish_solve_batch<KK>), dim3(j1 - j0), dim3(1024), 0, s, d_solve + j0, d_part, 0, d_mom,
                                                         mom_stride, 1, b->d_coeffs, d_tab, d_st));
        MCX_HIP(h, hipGetLastError());
        return 0;
    }
    size_t l = std::upper_bound(bt.launch_begin.begin(), bt.launch_begin.end(), (int32_t)j0) - bt.launch_begin.begin() - 1;
    for (; l + 1 < bt.launch_begin.size() && bt.launch_begin[l] < j1; ++l) {
        const int a0 = bt.launch_begin[l], nj = bt.launch_begin[l + 1] - a0;
        K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_step_batch<KK>), dim3(bt.tiles, nj), dim3(MCX_BLOCK), 0, s, d_step + a0));
        K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_finish_solve_batch<KK>), dim3(nj), dim3(1024), 0, s, d_solve + a0, d_part, 1,
                                          d_mom + (size_t)(a0 - j0) * mom_stride, mom_stride, do_solve, b->d_coeffs, d_tab, d_st));
        MCX_HIP(h, hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" int mcx_storage_lsm_step_batch(mcx_handle* h, const mcx_book* b, const mcx_storage* const* storages, int32_t n_storages,
                                          const mcx_storage_lsm_job* h_jobs, int32_t n_jobs, const double* d_paths, int64_t n_paths,
                                          int64_t ld, double* d_W, int64_t ld_w, int64_t w_len, double* d_moments, int64_t mom_stride,
                                          int32_t flags, void* stream)
{
    if (!h || !b || !storages || !h_jobs || !d_paths || !d_W || !d_moments) return -1;
    if (n_jobs <= 0) return 0;
    const int32_t step_begin[2] = {0, n_jobs};
    K6Batch bt;
    const int rc = k6_batch_build(h, b, storages, n_storages, h_jobs, step_begin, 1, d_paths, n_paths, ld, d_W, ld_w, w_len, flags,
                                  "mcx_storage_lsm_step_batch", bt);
    if (rc != 0) return rc;
    if (mom_stride < bt.nm_max) MCX_FAIL(h, -2, "mcx_storage_lsm_step_batch: mom_stride %lld < %d moments of a job", (long long)mom_stride, bt.nm_max);
    hipStream_t s = (hipStream_t)stream;
    const size_t step_bytes = sizeof(K6StepArgs) * (size_t)n_jobs, solve_bytes = sizeof(K6BatchSolve) * (size_t)n_jobs;
    double* d_part = (double*)mcx_scratch(h, 2, sizeof(double) * bt.part_doubles);
    unsigned char* d_fb = (unsigned char*)mcx_scratch(h, 1, step_bytes + solve_bytes);
    if (!d_part || !d_fb) return -100;
    k6_batch_place(bt, d_part);
    const K6StepArgs* d_step = (const K6StepArgs*)mcx_upload_call_data(h, bt.step.data(), step_bytes, d_fb, s);
    const K6BatchSolve* d_solve = (const K6BatchSolve*)mcx_upload_call_data(h, bt.solve.data(), solve_bytes, d_fb + step_bytes, s);
    if (!d_step || !d_solve) return -100;
    return k6_batch_step(h, b, bt, d_step, d_solve, 0, n_jobs, d_part, d_moments, mom_stride, 0, nullptr, nullptr, s);     // stream-ordered
}

extern "C" int mcx_storage_lsm_solve_batch(mcx_handle* h, mcx_book* b, const mcx_storage* const* storages, int32_t n_storages,
                                           const mcx_storage_lsm_job* h_jobs, int32_t n_jobs, double* d_moments, int64_t mom_stride,
                                           double* d_coeff_table, int32_t* d_status, void* stream)
{
    if (!h || !b || !storages || !h_jobs || !d_moments || !d_status) return -1;
    if (n_jobs <= 0) return 0;
    const int K = b->n_basis;
    if (K < 1 || K > 6) MCX_FAIL(h, -3, "mcx_storage_lsm_solve_batch: unsupported basis size %d", K);
    std::vector<K6BatchSolve> solve((size_t)n_jobs);
    std::vector<int32_t> seen((size_t)(n_storages > 0 ? n_storages : 0), -2);
    int64_t tab = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const mcx_storage_lsm_job& q = h_jobs[j];
        if (int rc = k6_check_job(h, b, storages, n_storages, q, j, -1, seen, "mcx_storage_lsm_solve_batch")) return rc;
        const int S = storages[q.storage]->n_states;
        if ((2 * K - 1) + S * K > mom_stride) MCX_FAIL(h, -2, "mcx_storage_lsm_solve_batch: job %d: mom_stride too small", j);
        K6BatchSolve& v = solve[j];
        memset(&v, 0, sizeof(v));
        v.q = k6_fill_solve(q, S, j);
        v.tab_off = tab;
        tab += (int64_t)S * K;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t solve_bytes = sizeof(K6BatchSolve) * (size_t)n_jobs;
    void* d_fb = mcx_scratch(h, 1, solve_bytes);
    if (!d_fb) return -100;
    const K6BatchSolve* d_solve = (const K6BatchSolve*)mcx_upload_call_data(h, solve.data(), solve_bytes, d_fb, s);
    if (!d_solve) return -100;
    K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_finish_solve_batch<KK>), dim3(n_jobs), dim3(1024), 0, s, d_solve, (const double*)nullptr, 0, d_moments,
                                      mom_stride, 1, b->d_coeffs, d_coeff_table, d_status));
    MCX_HIP(h, hipGetLastError());
    return 0;          // stream-ordered
}

extern "C" int mcx_storage_lsm_run_batch(mcx_handle* h, mcx_book* b, const mcx_storage* const* storages, int32_t n_storages,
                                         const mcx_storage_lsm_job* h_jobs, const int32_t* h_step_begin, int32_t n_steps,
                                         const double* d_paths, int64_t n_paths, int64_t ld, double* d_W, int64_t ld_w, int64_t w_len,
                                         double* h_coeffs, int32_t* h_status, int32_t flags, void* stream)
{
    if (!h || !b || !storages || !h_jobs || !h_step_begin || !d_paths || !d_W || !h_coeffs || !h_status) return -1;
    if (n_steps <= 0) return 0;
    K6Batch bt;
    int rc = k6_batch_build(h, b, storages, n_storages, h_jobs, h_step_begin, n_steps, d_paths, n_paths, ld, d_W, ld_w, w_len, flags,
                            "mcx_storage_lsm_run_batch", bt);
    if (rc != 0) return rc;
    const int n_jobs = h_step_begin[n_steps];
    if (n_jobs <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t stride = bt.nm_max;
    const size_t step_bytes = sizeof(K6StepArgs) * (size_t)n_jobs, solve_bytes = sizeof(K6BatchSolve) * (size_t)n_jobs;
    const size_t tab_bytes = sizeof(double) * (size_t)bt.tab_doubles, st_bytes = sizeof(int32_t) * (size_t)n_jobs;
    // slot 1: both job tables, the packed coefficient table, the status words; slot 2: partials; slot 3: the moments of a step
    unsigned char* d_tabs = (unsigned char*)mcx_scratch(h, 1, step_bytes + solve_bytes + tab_bytes + st_bytes);
    double* d_part = (double*)mcx_scratch(h, 2, sizeof(double) * bt.part_doubles);
    double* d_mom = (double*)mcx_scratch(h, 3, sizeof(double) * (size_t)bt.widest * stride);
    if (!d_tabs || !d_part || !d_mom) return -100;
    k6_batch_place(bt, d_part);
    const K6StepArgs* d_step = (const K6StepArgs*)d_tabs;
    const K6BatchSolve* d_solve = (const K6BatchSolve*)(d_tabs + step_bytes);
    double* d_tab = (double*)(d_tabs + step_bytes + solve_bytes);
    int32_t* d_st = (int32_t*)(d_tabs + step_bytes + solve_bytes + tab_bytes);
    // uploaded once, before the first launch (the host vectors die with this call, which ends in a synchronisation)
    MCX_HIP(h, hipMemcpyAsync(d_tabs, bt.step.data(), step_bytes, hipMemcpyHostToDevice, s));
    MCX_HIP(h, hipMemcpyAsync(d_tabs + step_bytes, bt.solve.data(), solve_bytes, hipMemcpyHostToDevice, s));
    const bool multi = h->comm && h->comm_ranks > 1;
    for (int t = 0; t < n_steps && rc == 0; ++t) {
        const int j0 = h_step_begin[t], j1 = h_step_begin[t + 1];
        if (j1 <= j0) continue;
        rc = k6_batch_step(h, b, bt, d_step, d_solve, j0, j1, d_part, d_mom, stride, multi ? 0 : 1, d_tab, d_st, s);
        if (rc != 0 || !multi) continue;
        rc = mcx_allreduce_f64(h, d_mom, (int64_t)(j1 - j0) * stride, stream);          // ONE collective per step, stream-ordered
        if (rc != 0) break;
        const int K = b->n_basis;
        K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_finish_solve_batch<KK>), dim3(j1 - j0), dim3(1024), 0, s, d_solve + j0, (const double*)nullptr, 0,
                                          d_mom, stride, 1, b->d_coeffs, d_tab, d_st));
        if (hipGetLastError() != hipSuccess) { h->err = "mcx_storage_lsm_run_batch: launch failed"; rc = -100; }
    }
    if (rc == 0 && (hipMemcpyAsync(h_coeffs, d_tab, tab_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipMemcpyAsync(h_status, d_st, st_bytes, hipMemcpyDeviceToHost, s) != hipSuccess)) { h->err = "mcx_storage_lsm_run_batch: copy failed"; rc = -100; }
    if (hipStreamSynchronize(s) != hipSuccess && rc == 0) { h->err = "mcx_storage_lsm_run_batch: synchronise failed"; rc = -100; }
    return rc;
}

extern "C" int mcx_storage_eval(mcx_handle* h, const mcx_book* b, const mcx_storage* st, const mcx_storage_op* h_ops, int32_t n_ops,
                                const double* d_paths, int64_t n_paths, int64_t ld, double* d_cfs, double* d_expo, int64_t ld_out,
                                void* stream)
{
    if (!h || !b || !st || !h_ops || !d_paths) return -1;
    if (n_paths <= 0 || n_ops <= 0) return 0;
    if (st->n_basis != b->n_basis || st->n_coeffs != b->n_coeffs) MCX_FAIL(h, -2, "mcx_storage_eval: the storage was created on another book");
    if (ld < n_paths || ld_out < n_paths) MCX_FAIL(h, -2, "mcx_storage_eval: leading dimension < n_paths");
    if (st->netting_set >= b->n_netting_sets) MCX_FAIL(h, -2, "mcx_storage_eval: netting set out of range");
    const int K = st->n_basis, S = st->n_states;
    for (int q = 0; q < n_ops; ++q) {
        const mcx_storage_op& o = h_ops[q];
        if (o.kind == 0) {
            if (o.index < 0 || o.index >= st->n_dates) MCX_FAIL(h, -2, "mcx_storage_eval: op %d: action date out of range", q);
        } else if (o.kind == 1) {
            if (!d_expo || o.index < 0 || o.index >= b->n_expo_rows) MCX_FAIL(h, -2, "mcx_storage_eval: op %d: exposure row out of range", q);
            if (o.num_atom < 0 || o.num_atom >= b->n_atoms || o.x_atom < 0 || o.x_atom >= b->n_atoms)
                MCX_FAIL(h, -2, "mcx_storage_eval: op %d: atom out of range", q);
            if (o.coeff_off < 0 || o.coeff_off + (int64_t)S * K > b->n_coeffs) MCX_FAIL(h, -2, "mcx_storage_eval: op %d: coefficient block out of range", q);
        } else MCX_FAIL(h, -2, "mcx_storage_eval: op %d: bad kind", q);
    }
    hipStream_t s = (hipStream_t)stream;
    const mcx_storage_op* d_ops = (const mcx_storage_op*)mcx_stage_small(h, h_ops, sizeof(mcx_storage_op) * (size_t)n_ops, s);
    if (!d_ops) return -100;
    K6EvalArgs a;
    a.paths = d_paths; a.dates = st->d_dates; a.ops = d_ops; a.atoms = b->d_atoms; a.coeffs = b->d_coeffs;
    a.cfs = d_cfs ? d_cfs + (size_t)st->netting_set * ld_out : nullptr;
    a.expo = d_expo ? d_expo + (size_t)st->netting_set * b->n_expo_rows * ld_out : nullptr;
    a.n = n_paths; a.ld = ld; a.ld_out = ld_out; a.n_ops = n_ops; a.S = S; a.n_state = b->n_state; a.pad = 0;
    const int grid = (int)((n_paths + MCX_BLOCK - 1) / MCX_BLOCK);
    K6_DISPATCH(K, 6, hipLaunchKernelGGL((k6_eval<KK>), dim3(grid), dim3(MCX_BLOCK), 0, s, a));
    MCX_HIP(h, hipGetLastError());
    return 0;          // stream-ordered
}
