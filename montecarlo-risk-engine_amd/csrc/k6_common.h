// k6_common.h — the primal arithmetic and the date record of the gas storage, shared by k6_storage.hip (primal kernels) and
// kt_storage.hip (their tangent images).  Every primal value of either file is formed HERE, by one definition: image 0 of the
// tangent kernels equals the primal kernels' results bit for bit by construction, so no decision can differ.  gfx950 only.
#pragma once
#include "mcx_internal.h"

#define K6_MAX_S MCX_STORAGE_MAX_STATES
#define K6_MAX_KNOTS MCX_STORAGE_MAX_KNOTS

// ---- primitives ------------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ double k6_poly(const double* __restrict__ c, double x)
{
    double v = 0.0, xp = 1.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { v = fma(c[k], xp, v); xp *= x; }
    return v;
}
// the same with a wave-uniform coefficient row (scalar loads)
template <int K>
__device__ __forceinline__ double k6_poly_uniform(const double* __restrict__ c, double x)
{
    double v = 0.0, xp = 1.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { v = fma(ldk(c + k), xp, v); xp *= x; }
    return v;
}

// piecewise-linear rate at volume v (storage_helpers.py interpolate_rate_tensor): segment = the last knot below v, clamped to
// the first / last segment; weight 0 where the segment's knots coincide under torch.isclose; flat outside the knots.  The knots
// are wave-uniform, v is per lane: selects, no dynamic indexing.  (Volumes carry no parameter dependence: no tangent.)
__device__ __forceinline__ double k6_rate(const double* __restrict__ xs, const double* __restrict__ rs, int n, double v)
{
    if (n == 1) return rs[0];
    double x0 = xs[0], x1 = xs[1], y0 = rs[0], y1 = rs[1];
    for (int j = 1; j < n - 1; ++j) {
        const bool m = xs[j] < v;
        x0 = m ? xs[j] : x0; x1 = m ? xs[j + 1] : x1;
        y0 = m ? rs[j] : y0; y1 = m ? rs[j + 1] : y1;
    }
    const bool close = fabs(x0 - x1) <= 1e-8 + 1e-5 * fabs(x1);
    const double w = close ? 0.0 : (v - x0) / (x1 - x0);
    double r = y0 + w * (y1 - y0);
    r = v <= xs[0] ? rs[0] : r;
    r = v >= xs[n - 1] ? rs[n - 1] : r;
    return r;
}

// polynomial grid of the staged coefficient block interpolated at a per-lane state
template <int K>
__device__ __forceinline__ double k6_lerp_grid(const double* __restrict__ sc, int S, double state, double x)
{
    const double b = fmin(fmax(state, 0.0), (double)(S - 1));
    const double fl = floor(b), w = b - fl;
    const int lo = (int)fl, hi = (int)ceil(b);
    const double g_lo = k6_poly<K>(sc + lo * K, x), g_hi = k6_poly<K>(sc + hi * K, x);
    return g_lo + w * (g_hi - g_lo);
}

// ---- backward step ---------------------------------------------------------------------------------------------------
// one candidate of an integer start state: (next state, dv) wave-uniform, the price per lane.  coeffs: the [S][K] block of the
// rolled date (unused when is_last), W_old: [S][ld_w].  -> cash, value, cached tail, and where the tail was read (rows lo, hi
// at weight w: the tangent kernel reads the tail's tangent there, the primal kernel ignores them)
template <int K>
__device__ __forceinline__ void k6_step_candidate(const double* __restrict__ coeffs, const double* __restrict__ W_old, int64_t ld_w, int S,
                                                  int is_last, double ns, double dv, double price, double spot, int64_t i,
                                                  double& cash, double& value, double& tail, int& lo, int& hi, double& w)
{
    const double b = fmin(fmax(ns, 0.0), (double)(S - 1));
    const double fl = floor(b);
    w = b - fl;
    lo = (int)fl; hi = (int)ceil(b);
    double cont = 0.0;
    if (!is_last) {
        const double g_lo = k6_poly_uniform<K>(coeffs + lo * K, spot);
        const double g_hi = hi != lo ? k6_poly_uniform<K>(coeffs + hi * K, spot) : g_lo;
        cont = g_lo + w * (g_hi - g_lo);
    }
    const double w_lo = W_old[(int64_t)lo * ld_w + i];
    const double w_hi = hi != lo ? W_old[(int64_t)hi * ld_w + i] : w_lo;
    tail = w_lo + w * (w_hi - w_lo);
    cash = -dv * price;
    value = cash + cont;
}

// ---- main simulation -------------------------------------------------------------------------------------------------
struct KTSAtom { DevAtom a; int32_t id, pad; };      // the tangent kernels' atom: with its id (row of the atom derivatives)

template <class Atom>
struct K6DateT {                // device image of mcx_storage_date, atoms flattened
    double vmin, step, nvmin, nvmax, nscale, period, c_inj, c_wd;
    double inj_x[K6_MAX_KNOTS], inj_r[K6_MAX_KNOTS], wd_x[K6_MAX_KNOTS], wd_r[K6_MAX_KNOTS];
    Atom num, x;
    int64_t coeff_off;
    int32_t n_inj, n_wd, is_last, pad;
};
typedef K6DateT<DevAtom> K6Date;
typedef K6DateT<KTSAtom> KTSDate;
static_assert(sizeof(K6Date) % 8 == 0, "copied to LDS in dwords");
static_assert(sizeof(KTSDate) % 8 == 0, "copied to LDS in dwords");

struct K6Cand { double ns, cash, value, nv; };       // a candidate of the realised state: next state, cash, value, next volume

// one candidate of the realised state: next volume nv from volume v at `price`
template <int K, class Date>
__device__ __forceinline__ void k6_eval_candidate(const Date& d, const double* __restrict__ sc, int S, double nv, double v, double price,
                                                  double spot, K6Cand& c)
{
    c.nv = nv;
    c.ns = d.nscale == 0.0 ? 0.0 : (nv - d.nvmin) * d.nscale;
    c.cash = -(nv - v) * price;
    c.value = c.cash + (d.is_last ? 0.0 : k6_lerp_grid<K>(sc, S, c.ns, spot));
}

// the three candidates [inject, hold, withdraw] of the realised state at an action date: d the staged date record, sc its staged
// [S][K] coefficient block.  Exact ties between candidates are the rule (a full store: inject == hold): every candidate goes
// through ONE inline function, so tied candidates are bit-identical.  Returns the volume v of the state.
template <int K, class Date>
__device__ __forceinline__ double k6_eval_candidates(const Date& d, const double* __restrict__ sc, int S, double state, double spot,
                                                     K6Cand& inj, K6Cand& hold, K6Cand& wd)
{
    const double v = d.vmin + state * d.step;
    const double r_inj = k6_rate(d.inj_x, d.inj_r, d.n_inj, v), r_wd = k6_rate(d.wd_x, d.wd_r, d.n_wd, v);
    const double nv0 = fmin(v + r_inj * d.period, d.nvmax);
    const double nv1 = fmin(fmax(v, d.nvmin), d.nvmax);
    const double nv2 = fmax(v - r_wd * d.period, d.nvmin);
    const double p_inj = spot + d.c_inj, p_wd = spot - d.c_wd;
    k6_eval_candidate<K>(d, sc, S, nv0, v, p_inj, spot, inj);
    k6_eval_candidate<K>(d, sc, S, nv1, v, (nv1 - v) >= 0.0 ? p_inj : p_wd, spot, hold);
    k6_eval_candidate<K>(d, sc, S, nv2, v, p_wd, spot, wd);
    return v;
}

// ---- host ------------------------------------------------------------------------------------------------------------
inline void k6_set_atom(const mcx_book* b, int id, DevAtom& o) { o = mcx_flat_atom(b->h_atoms[id]); }
inline void k6_set_atom(const mcx_book* b, int id, KTSAtom& o) { o.a = mcx_flat_atom(b->h_atoms[id]); o.id = id; o.pad = 0; }

// the descriptor of a storage on book b (who: the entry point, for the message)
inline int k6_check_desc(mcx_handle* h, const mcx_book* b, const mcx_storage_desc* d, const char* who)
{
    if (!d->dates || !d->trans) return -1;
    if (d->n_states < 2 || d->n_states > MCX_STORAGE_MAX_STATES) MCX_FAIL(h, -2, "%s: n_states %d outside [2, %d]", who, d->n_states, MCX_STORAGE_MAX_STATES);
    if (d->n_dates < 1) MCX_FAIL(h, -2, "%s: no action dates", who);
    if (d->netting_set < 0 || d->netting_set >= b->n_netting_sets) MCX_FAIL(h, -2, "%s: netting set out of range", who);
    return 0;
}

// action date j of a checked descriptor
inline int k6_check_date(mcx_handle* h, const mcx_book* b, const mcx_storage_desc* d, int j, const char* who)
{
    const mcx_storage_date& q = d->dates[j];
    if (q.n_inj < 1 || q.n_inj > MCX_STORAGE_MAX_KNOTS || q.n_wd < 1 || q.n_wd > MCX_STORAGE_MAX_KNOTS)
        MCX_FAIL(h, -3, "%s: date %d: knot count outside [1, %d]", who, j, MCX_STORAGE_MAX_KNOTS);
    if (q.num_atom < 0 || q.num_atom >= b->n_atoms || q.x_atom < 0 || q.x_atom >= b->n_atoms) MCX_FAIL(h, -3, "%s: date %d: atom out of range", who, j);
    if (q.coeff_off < 0 || q.coeff_off + (int64_t)d->n_states * b->n_basis > b->n_coeffs)
        MCX_FAIL(h, -3, "%s: date %d: coefficient block out of range", who, j);
    return 0;
}

// the device record of a checked date
template <class Atom>
void k6_fill_date(const mcx_book* b, const mcx_storage_date& q, K6DateT<Atom>& o)
{
    memset(&o, 0, sizeof(o));
    o.vmin = q.vmin; o.step = q.step; o.nvmin = q.next_vmin; o.nvmax = q.next_vmax; o.nscale = q.next_scale;
    o.period = q.period; o.c_inj = q.c_inj; o.c_wd = q.c_wd;
    memcpy(o.inj_x, q.inj_x, sizeof(o.inj_x)); memcpy(o.inj_r, q.inj_r, sizeof(o.inj_r));
    memcpy(o.wd_x, q.wd_x, sizeof(o.wd_x)); memcpy(o.wd_r, q.wd_r, sizeof(o.wd_r));
    k6_set_atom(b, q.num_atom, o.num); k6_set_atom(b, q.x_atom, o.x);
    o.coeff_off = q.coeff_off; o.n_inj = q.n_inj; o.n_wd = q.n_wd; o.is_last = q.is_last ? 1 : 0;
}

// launch of a kernel template on the basis size: CALL with KK = K for 1 <= K <= KMAX (4 or 6), nothing otherwise
#define K6_DISPATCH(K, KMAX, ...) MCX_DISPATCH(KK, K, KMAX, __VA_ARGS__)
