// kf_common.h — records, device helpers and the straight-line date program (lean_date) shared by the fused main-pass kernels
// (kf_fused.hip: event interpreter and evaluation-from-paths pass; kf_lean.hip: the straight-line one-launch kernel).  gfx950 only.
#pragma once
#include <cstddef>
#include "mcx_device.h"



enum { FA_EXP = 1, FA_AFFINE = 2 };      // FAtom::parts: the atom has an exponential term (b != 0), an affine term (a or d != 0)
struct FAtom {             // value = a + d*x + b*exp(c0 + c1*x), x = register `reg` of the lane (reg < 0: x = 0)
    int32_t reg, parts;
    double a, d, b, c0, c1;
};
struct FTerm { double w; FAtom atom; };
enum { FE_SAME_NUM = 2 };  // FEvent::flags (beside the book's own event flags): same numeraire as the previous event of the date
struct FEvent {
    int32_t kind, flags;
    int32_t term_begin, term_end;
    int32_t coeff_off, row;
    int32_t ns, sidx;          // netting-set slot (0..3), stateful-product slot (0..3) or -1
    int32_t init_state, n_states;      // of the event's product
    double strike, sign;
    double aux[4];
    FAtom num, x;
};
struct FMetricOp {             // one (netting set, metric date) pair, executed after the date's events
    int32_t ns, m;
    int32_t rec_profile;       // record index of relu(u) (rec+1 = -relu(-u)), -1: no profiles
    int32_t has_cva;           // 1: m < n_dates-1 and CVA wanted
    double threshold;
    FAtom surv, cond;
};

static_assert(sizeof(FAtom) == 48 && sizeof(FEvent) == 184 && sizeof(FMetricOp) == 120, "program records are uploaded byte for byte");

struct ChunkHeader { int32_t n_ev, n_mop, n_terms, bytes; };

// FastDate::flags.  The values are the public MCX_FD_* (include/mcx.h), which mcx_fused_describe reports per date.
enum {
    FD_CASH = MCX_FD_CASH,                // cashflows (k0, k1, t_*) or a plain option payoff: feeds the PV record / cashflow output
    FD_EXPO = MCX_FD_EXPO,                // polynomial exposure in x_a + x_d reg[x_reg], rows coeff_off0 / coeff_off1
    FD_CVA = MCX_FD_CVA,                  // CVA increment: survival s_*, conditional survival c_*
    FD_PROFILE = MCX_FD_PROFILE,          // EPE / ENE records rec_profile, rec_profile + 1
    FD_CONST_NUM = MCX_FD_CONST_NUM,      // constant numeraire: 1/numeraire = ni_c0
    FD_METRIC = MCX_FD_METRIC,            // a metric op is present (thr, and FD_PROFILE and / or FD_CVA)
    FD_MERGED = MCX_FD_MERGED,            // the CVA increment may use the merged discount x survival factor (m_*): no threshold,
                                          //     no EPE / ENE record on this date
    FD_EXERCISE = MCX_FD_EXERCISE,        // exercise event of the book's ONE two-state exercise product (ex_*)
    FD_STATE_EXPO = MCX_FD_STATE_EXPO,    // the exposure's coefficient row is indexed by the lane's exercise state
    FD_OPTION = MCX_FD_OPTION,            // the cash value is a plain option payoff (op_strike, op_sign)
    FD_EX_VPOLY = MCX_FD_EX_VPOLY         // the exercise value is also ONE verified polynomial (ex_p_*)
};

// Straight-line record of a date whose program is the common linear-book shape (one netting set; cashflows that are an
// affine term + <= 4 exponential terms over a pure-exponential or constant numeraire, or a plain option payoff; polynomial
// exposures; the exercise event of one two-state product; an optional threshold / EPE-ENE record / CVA increment).  Such a
// date runs ~130 instructions of branch-light code with every control field in SGPRs instead of ~500 instructions of event
// interpretation; any other date uses the interpreter.
struct FastDate {
    // ---- hot head (FastDateHot below is a view of these 144 bytes: ONE batch of scalar loads at the top of a date) ----
    int32_t valid, flags;            // valid: 0 interpreted, 1 straight-line (lean_date, in kf_lean and kf_fused alike)
                                     // flags: FD_* above
    int32_t ni_reg, lin_reg, n_exp, x_reg, coeff_off0, coeff_off1, rec_profile, s_reg, c_reg, pad;
    int32_t t_reg[4];
    double x_a, x_d;                 // explanatory x = x_a + x_d * reg[x_reg]
    double c_a, c_b, c_c0, c_c1;     // S(t,t+) cond = c_a + c_b exp(c_c0 + c_c1 reg[c_reg])
    double m_b, m_c0, m_n1, m_s1;    // S(0,t) / numeraire = m_b exp(m_c0 + m_n1 reg[ni_reg] + m_s1 reg[s_reg])   (FD_MERGED)
    // ---- the rest: read at the point of use ----
    double ni_c0, ni_c1;             // 1/numeraire = exp(ni_c0 + ni_c1 x)   (FD_CONST_NUM: = ni_c0)
    double k0, k1;                   // cash affine part k0 + k1 * reg[lin_reg]
    double t_w[4], t_c0[4], t_c1[4];
    double thr;
    double s_b, s_c0, s_c1;          // S(0,t)       = s_b exp(s_c0 + s_c1 reg[s_reg])
    // FD_EXERCISE: exercise event of the book's ONE two-state exercise product (bermudan_option.py:93-131): immediate value
    // max(ex_sign (ex_k0 + ex_k1 reg[ex_lin_reg] + sum_j w_j exp(c0_j + c1_j reg[r_j]) - ex_strike), 0) over the LeanTerm range
    // [ex_term_off, ex_term_off + ex_n); continuation = polynomial (row of state 1 at ex_coeff_off + n_basis) in ex_x_a + ex_x_d reg[ex_x_reg]
    // FD_STATE_EXPO: the exposure polynomial's coefficient row is indexed by the lane's exercise state (coeff_off0 + state * n_basis)
    int32_t ex_n, ex_term_off, ex_coeff_off, ex_x_reg, ex_lin_reg, ex_pad;
    double ex_k0, ex_k1, ex_strike, ex_sign, ex_x_a, ex_x_d;
    // FD_OPTION: the date's cash value is a plain option payoff (european_option.py:45-68): max(op_sign (value - op_strike), 0)
    double op_strike, op_sign;
    // FD_EX_VPOLY: the exercise value (affine part, constants and every exponential term) is also available as ONE verified polynomial of
    // reg[ex_p_reg] (mcx_vpoly.hip): p(t), t = fma(x, ex_p_ih, ex_p_ms), ex_p_blk blocks of 4 coefficients at vcoef + ex_p_off, valid
    // for ex_p_lo <= x <= ex_p_hi; a wave that holds a path outside runs the LeanTerm loop
    double ex_p_lo, ex_p_hi, ex_p_ms, ex_p_ih;
    int32_t ex_p_off, ex_p_blk, ex_p_reg, ex_p_pad;
};
// the head of a FastDate as one record (what a CVA-only date reads: lean_date below)
struct FastDateHot {
    int32_t valid, flags;
    int32_t ni_reg, lin_reg, n_exp, x_reg, coeff_off0, coeff_off1, rec_profile, s_reg, c_reg, pad;
    int32_t t_reg[4];
    double x_a, x_d;
    double c_a, c_b, c_c0, c_c1;
    double m_b, m_c0, m_n1, m_s1;
};
static_assert(sizeof(FastDateHot) == 144 && offsetof(FastDate, ni_c0) == sizeof(FastDateHot), "FastDateHot must mirror the head of FastDate");
struct LeanTerm { double w, c0, c1; int32_t reg, pad; };     // w exp(c0 + c1 reg[reg]), read through scalar loads

// The CVA-only date of a Vasicek + CIR++ (Euler) book, for the cva-date instantiation of kf_lean (kf_lean.hip lean_date_cva).
// FastDateCva is what mcx_fused_create builds: the ten doubles of the date (the FastDate fields of the same names) and the offsets
// of its regression rows in the book's coefficient table (-1: absent).  The coefficients change between runs (LSM), so the kernel
// prologue gathers them and stages every date as one 128-byte FastDateCvaLds in LDS.  The state registers are the signature's
// canonical layout (FDC_X_REG ...), so neither record carries any.
struct alignas(16) FastDateCva {
    double m_s1, m_n1, m_c0, m_b;    // S(0,t) / numeraire = m_b exp(m_c0 + m_n1 reg[FDC_NI_REG] + m_s1 reg[FDC_S_REG])
    double c_c1, c_c0, c_a, c_b;     // S(t,t+) cond = c_a + c_b exp(c_c0 + c_c1 reg[FDC_C_REG])
    double x_d, x_a;                 // x = x_a + x_d reg[FDC_X_REG]
    int32_t coeff_off0, coeff_off1, pad[2];
};
// An absent row is a row of zeros: it adds +0.0 to the exposure, which leaves it unchanged for a finite state (the sum starts
// at 0.0 + first row, so it is never -0.0).  A date with no effect on the CVA (no metric op, no cash consumer) is an all-zero
// record: its increment is fma(0, 0, cva) = cva.
struct alignas(16) FastDateCvaLds {
    double m_s1, m_n1, m_c0, m_b, c_c1, c_c0, c_a, c_b, x_d, x_a;
    double row0[3], row1[3];
};
#define FDC_HEAD 10                  // doubles of FastDateCva copied as they are, in this order
static_assert(sizeof(FastDateCva) == 96 && offsetof(FastDateCva, coeff_off0) == FDC_HEAD * sizeof(double), "FastDateCva layout");
static_assert(sizeof(FastDateCvaLds) == 128 && offsetof(FastDateCvaLds, row0) == FDC_HEAD * sizeof(double), "FastDateCvaLds layout");
// canonical registers of SIG_VAS_CIR_E: Vasicek (r, log B) in slot 0, CIR++ (lambda, integral of lambda) in slot 1
enum { FDC_X_REG = 0, FDC_NI_REG = 1, FDC_C_REG = 2, FDC_S_REG = 3 };

struct FusedArgs {
    K1Args k1;
    const FastDate* __restrict__ fast;        // [n_dates]
    const FastDateCva* __restrict__ cva_dates;    // [n_dates] or nullptr: the book runs the cva-date kernel (kf_lean.hip)
    const LeanTerm* __restrict__ lterms;      // exponential terms of the exercise values (FastDate::ex_term_off)
    const double* __restrict__ vcoef;         // coefficients of the exercise-value polynomials (FastDate::ex_p_off), one spare block at the end
    const unsigned char* __restrict__ prog;   // per-date program chunks (header | events | terms | metric ops)
    const int32_t* __restrict__ date_off;     // [n_dates+1] byte offset of each date's chunk (16-byte aligned)
    const int32_t* __restrict__ date_row;     // [n_dates] exposure row of this timeline date or -1
    const double* __restrict__ coeffs;
    double* __restrict__ cfs;                 // nullable [NS][ld_out]
    double* __restrict__ expo;                // nullable [NS][n_expo_rows][ld_out]
    double* __restrict__ partials;            // [gridDim.x][n_rec][4]
    int64_t ld_out;
    int32_t n_dates, n_basis, n_ns, n_rec, n_expo_rows, n_stateful, chunk_cap, pad;
    int32_t rec_pv[MCX_FUSED_MAX_NS];         // record index of the PV record of ns slot k, or -1
    int32_t rec_cva[MCX_FUSED_MAX_NS];
    double lgd[MCX_FUSED_MAX_NS];
    int32_t init_state[MCX_FUSED_MAX_STATEFUL];
};

// merge of two (count, mean, centred second moment) triples (Chan, Golub, LeVeque pairwise update)
__device__ __forceinline__ void chan_merge(double& N, double& mean, double& M2, double n, double m, double q)
{
    if (n <= 0.0) return;
    if (N == 0.0) { N = n; mean = m; M2 = q; return; }
    const double delta = m - mean, tot = N + n;
    mean += delta * n / tot;
    M2 += q + delta * delta * N * n / tot;
    N = tot;
}

#define RFL(x) __builtin_amdgcn_readfirstlane(x)

template <int NREG>
__device__ __forceinline__ double f_atom(const FAtom& a, const double (&reg)[NREG])
{
    // the program lives in LDS, so its fields arrive in VGPRs; the CONTROL fields are made wave-uniform SGPRs
    // (v_readfirstlane) so that selects / branches are scalar instead of exec-masked divergent code
    const int r = RFL(a.reg), fl = RFL(a.parts);
    const double x = r >= 0 ? reg[r] : 0.0;             // uniform dynamic index -> M0-relative VGPR read (v_movrels)
    double v = (fl & FA_AFFINE) ? fma(a.d, x, a.a) : 0.0;
    if (fl & FA_EXP) v = fma(a.b, mcx_exp(fma(a.c1, x, a.c0)), v);
    return v;
}

// coefficients of a STATELESS product are the same for every lane: wave-uniform offset -> scalar loads (s_load through the
// scalar cache) instead of a dependent per-lane global load with L2 latency on every exposure date
__device__ __forceinline__ double f_poly_uniform(const double* __restrict__ coeffs, int off_vgpr, int K, double x)
{
    const double* __restrict__ c = coeffs + __builtin_amdgcn_readfirstlane(off_vgpr);
    double v = 0.0, xp = 1.0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) { v = fma(ldk(c + k), xp, v); xp *= x; }
    return v;
}

__device__ __forceinline__ double f_poly(const double* __restrict__ c, int K, double x)
{
    double v = 0.0, xp = 1.0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) { v = fma(c[k], xp, v); xp *= x; }
    return v;
}

template <int NREG>
__device__ __forceinline__ double f_regsel(int r, const double (&reg)[NREG])      // r is wave-uniform (SGPR)
{
    return r >= 0 ? reg[r] : 0.0;       // uniform dynamic index -> v_movrels (M0-relative VGPR read), no select chain
}

// ---- the date program of a FastDate record in kf_lean.hip (lean_date, PPL paths per lane) ----

#define FD(x) ldk(&fp->x)

// the kernel arguments as seen from one code region: the kernarg segment (explicit arguments start at offset 0) behind a
// region zero
typedef const MCX_KONST FusedArgs KArgs;
__device__ __forceinline__ KArgs& kargs_region(int z)
{
    return *(KArgs*)((const MCX_KONST char*)__builtin_amdgcn_kernarg_segment_ptr() + z);
}

// polynomial in the raw explanatory variable with wave-uniform coefficients (scalar loads); K == 3 is the default
// PolyomialRegression(degree=2) of the reference (controller.py:35)
template <int PPL>
__device__ __forceinline__ void lean_poly_add(const double* __restrict__ c, int K, const double (&x)[PPL], double (&p)[PPL])
{
    if (K == 3) {
        const double c0 = ldk(c), c1 = ldk(c + 1), c2 = ldk(c + 2);
#pragma unroll
        for (int q = 0; q < PPL; ++q) p[q] += fma(fma(c2, x[q], c1), x[q], c0);
    } else {
        double v[PPL];
#pragma unroll
        for (int q = 0; q < PPL; ++q) v[q] = 0.0;
#pragma unroll 1
        for (int k = K - 1; k >= 0; --k) {
            const double ck = ldk(c + k);
#pragma unroll
            for (int q = 0; q < PPL; ++q) v[q] = fma(v[q], x[q], ck);
        }
#pragma unroll
        for (int q = 0; q < PPL; ++q) p[q] += v[q];
    }
}

// LDS record area: shift[n_rec] | acc[4 waves][n_rec][2]
template <int PPL>
__device__ __forceinline__ void lean_record(const double (&v)[PPL], const bool (&live)[PPL], int rec, int n_rec, bool first_tile,
                                            double* __restrict__ lds)
{
    if (first_tile) {                      // block-uniform: the first path the block sees fixes the record's shift
        __syncthreads();
        if (threadIdx.x == 0) lds[rec] = v[0];
        __syncthreads();
    }
    const double c = lds[rec];
    double d1 = 0.0, d2 = 0.0;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const double d = live[q] ? v[q] - c : 0.0;
        d1 += d;
        d2 = fma(d, d, d2);
    }
    const double s1 = wave_sum(d1), s2 = wave_sum(d2);
    if ((threadIdx.x & 63) == 0) {
        double* acc = lds + n_rec + ((threadIdx.x >> 6) * n_rec + rec) * 2;
        acc[0] += s1;
        acc[1] += s2;
    }
}

template <int NSLOT, int SIG, int PPL, bool STORE>
__device__ __forceinline__ void lean_date(int t, const int64_t (&i)[PPL], const bool (&live)[PPL], bool first_tile,
                                          double* __restrict__ lds, const double (&reg)[PPL][2 * NSLOT], double (&cfs)[PPL], double (&cva)[PPL],
                                          int (&est)[PPL], const double* __restrict__ etab)
{
    // (state registers are indexed by wave-uniform record fields: M0-relative VGPR reads; mcx_fused_create binds an absent
    // reference to register 0 with a zero coefficient, so no range test is needed)
    const int zd = mcx_region_zero();                  // arguments, date record and exp coefficients: live in this block only
    KArgs& a = kargs_region(zd);
    const FastDate* __restrict__ fp = a.fast + t;
    const auto& k = a.k1;
    const mcx_expq_coef ec = mcx_expq_load(zd);       // exponentials: table of 2^(j/128) in LDS + degree-5 remainder
    // The CVA-only date (the config-3 shape: regression exposure, merged discount x survival factor, conditional default
    // probability — nothing stored, no cashflow consumer) in TWO rounds of scalar loads instead of one per branch of the general
    // program below: (1) the head of the record + the arguments, (2) the coefficient rows; and one round of LDS reads for its
    // two exponentials.  The waits of ~12 dependent scalar loads per date were a third of a wave's cycles at one or two waves
    // per SIMD.  Same arithmetic as the general path.
    // (the simulating kernel with two paths per lane at four waves per SIMD: measured slower — 52 SGPR spills around the date — than
    //  the general program below; the streaming kernel has no generator state to keep and is bound by the scalar unit, which the
    //  four SIMDs of a CU share: ~500 scalar instructions per date and wave of the general program cap it at ~4.3 TB/s)
    if ((PPL == 1 || !STORE) && !(STORE && k.paths)) {
        const FastDateHot hot = ldk_struct((const FastDateHot*)fp);
        const bool pure_cva = (hot.flags & (FD_MERGED | FD_EXERCISE | FD_STATE_EXPO | FD_EXPO)) == (FD_MERGED | FD_EXPO) && !((hot.flags & FD_CASH) && (a.cfs != nullptr || a.rec_pv[0] >= 0)) &&
                              a.expo == nullptr && a.n_basis == 3 && hot.c_b != 0.0;
        if (pure_cva) {
            const double* __restrict__ cf = a.coeffs;
            double c0[3] = {0.0, 0.0, 0.0}, c1[3] = {0.0, 0.0, 0.0};
            if (hot.coeff_off0 >= 0) {
#pragma unroll
                for (int j = 0; j < 3; ++j) c0[j] = ldk(cf + hot.coeff_off0 + j);
            }
            if (hot.coeff_off1 >= 0) {
#pragma unroll
                for (int j = 0; j < 3; ++j) c1[j] = ldk(cf + hot.coeff_off1 + j);
            }
            double xe[2 * PPL], ev[2 * PPL], p[PPL];
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                xe[2 * q] = fma(hot.m_s1, reg[q][hot.s_reg], fma(hot.m_n1, reg[q][hot.ni_reg], hot.m_c0));
                xe[2 * q + 1] = fma(hot.c_c1, reg[q][hot.c_reg], hot.c_c0);
            }
            mcx_exp_tab_n<2 * PPL>(xe, ev, etab, ec);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const double x = fma(hot.x_d, reg[q][hot.x_reg], hot.x_a);
                p[q] = 0.0;
                if (hot.coeff_off0 >= 0) p[q] += fma(fma(c0[2], x, c0[1]), x, c0[0]);
                if (hot.coeff_off1 >= 0) p[q] += fma(fma(c1[2], x, c1[1]), x, c1[0]);
                const double w = hot.m_b * ev[2 * q];
                const double cs = fma(hot.c_b, ev[2 * q + 1], hot.c_a);
                cva[q] = fma(fmax(p[q], 0.0), w * (1.0 - cs), cva[q]);
            }
            return;
        }
    }
    if (STORE && k.paths) {
#pragma unroll
        for (int q = 0; q < PPL; ++q) if (live[q]) sim_store_state<NSLOT, SIG>(k, t, i[q], reg[q]);
    }
    const int flags = FD(flags);
    // cashflows feed the PV record / the cashflow output only; a CVA / exposure-profile run skips them
    const bool want_cash = (flags & FD_CASH) && (a.cfs != nullptr || a.rec_pv[0] >= 0);
    // CVA-only date without threshold: relu(p / N) S (1 - Sc) = relu(p) (S / N) (1 - Sc), one exponential for S / N
    const bool merged = (flags & FD_MERGED) && !(flags & FD_EXERCISE) && !want_cash && a.expo == nullptr;
    double inv[PPL];
    if (!merged) {
        if (flags & FD_CONST_NUM) {
            const double c = FD(ni_c0);
#pragma unroll
            for (int q = 0; q < PPL; ++q) inv[q] = c;
        } else {
            const double c0 = FD(ni_c0), c1 = FD(ni_c1);
            const int r = FD(ni_reg);
#pragma unroll
            for (int q = 0; q < PPL; ++q) inv[q] = mcx_exp_tab(fma(c1, reg[q][r], c0), etab, ec);
        }
    }
    if (want_cash) {
        const double k0 = FD(k0), k1 = FD(k1);
        const int lr = FD(lin_reg), n_exp = FD(n_exp);
        double val[PPL];
#pragma unroll
        for (int q = 0; q < PPL; ++q) val[q] = fma(k1, reg[q][lr], k0);
#pragma unroll 1
        for (int j = 0; j < n_exp; ++j) {
            const double w = FD(t_w[j]), c0 = FD(t_c0[j]), c1 = FD(t_c1[j]);
            const int r = FD(t_reg[j]);
#pragma unroll
            for (int q = 0; q < PPL; ++q) val[q] = fma(w, mcx_exp_tab(fma(c1, reg[q][r], c0), etab, ec), val[q]);
        }
        if (flags & FD_OPTION) {                                 // plain option payoff (european_option.py:45-68)
            const double strike = FD(op_strike), sign = FD(op_sign);
#pragma unroll
            for (int q = 0; q < PPL; ++q) val[q] = fmax(sign * (val[q] - strike), 0.0);
        }
#pragma unroll
        for (int q = 0; q < PPL; ++q) cfs[q] = fma(val[q], inv[q], cfs[q]);
    }
    if (flags & FD_EXERCISE) {
        // exercise event of the two-state product (bermudan_option.py:93-131): exercise iff the immediate value exceeds the
        // regression continuation value and a right is left; the (up to ~64) exponential terms of the immediate value come
        // through scalar loads, one 32-byte record per term, and serve both paths of the lane
        const double strike = FD(ex_strike), sign = FD(ex_sign);
        double val[PPL];
        // the whole value as ONE verified polynomial of the state variable (mcx_vpoly.hip: ~20 multiply-adds for both paths of the
        // lane instead of ~15 VALU per term and path); a wave that holds a path outside the verified range runs the terms
        bool collapsed = false;
        if (flags & FD_EX_VPOLY) {
            const double lo = FD(ex_p_lo), hi = FD(ex_p_hi);
            const int pr = FD(ex_p_reg);
            bool in = true;
#pragma unroll
            for (int q = 0; q < PPL; ++q) in = in && reg[q][pr] >= lo && reg[q][pr] <= hi;
            if (__all(in)) {
                const double ms = FD(ex_p_ms), ih = FD(ex_p_ih);
                const int nb = FD(ex_p_blk);
                const VPolyBlk* __restrict__ blk = (const VPolyBlk*)(a.vcoef + FD(ex_p_off));
                double tt[PPL];
#pragma unroll
                for (int q = 0; q < PPL; ++q) { tt[q] = fma(reg[q][pr], ih, ms); val[q] = 0.0; }
                VPolyBlk c = ldk_struct(blk);
#pragma unroll 1
                for (int kb = 0; kb < nb; ++kb) {
                    const VPolyBlk nx = ldk_struct(blk + kb + 1);
#pragma unroll
                    for (int j = 0; j < MCX_VPOLY_BLK; ++j)
#pragma unroll
                        for (int q = 0; q < PPL; ++q) val[q] = fma(val[q], tt[q], c.c[j]);
                    c = nx;
                }
                collapsed = true;
            }
        }
        if (!collapsed) {
            const double k0 = FD(ex_k0), k1 = FD(ex_k1);
            const int lr = FD(ex_lin_reg), n_t = FD(ex_n);
            const LeanTerm* __restrict__ lt = a.lterms + FD(ex_term_off);
#pragma unroll
            for (int q = 0; q < PPL; ++q) val[q] = fma(k1, reg[q][lr], k0);
            // the next term's record is in flight while this term's two exponentials run (the table has one spare entry at its end)
            LeanTerm tm = ldk_struct(lt);
#pragma unroll 1
            for (int j = 0; j < n_t; ++j) {
                const LeanTerm nx = ldk_struct(lt + j + 1);
#pragma unroll
                for (int q = 0; q < PPL; ++q) val[q] = fma(tm.w, mcx_exp_tab(fma(tm.c1, reg[q][tm.reg], tm.c0), etab, ec), val[q]);
                tm = nx;
            }
        }
        const double xa = FD(ex_x_a), xd = FD(ex_x_d);
        const int xr = FD(ex_x_reg), co = FD(ex_coeff_off);
        double x[PPL], cont[PPL];
#pragma unroll
        for (int q = 0; q < PPL; ++q) { x[q] = fma(xd, reg[q][xr], xa); cont[q] = 0.0; }
        if (co >= 0) lean_poly_add<PPL>(a.coeffs + co + a.n_basis, a.n_basis, x, cont);      // row of state 1 (a right is left)
        const bool want_ex_cash = a.cfs != nullptr || a.rec_pv[0] >= 0;
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const double imm = fmax(sign * (val[q] - strike), 0.0);
            const bool ex = (imm > cont[q]) && (est[q] > 0);
            if (want_ex_cash) cfs[q] = ex ? fma(imm, inv[q], cfs[q]) : cfs[q];
            est[q] = ex ? est[q] - 1 : est[q];
        }
    }
    double p[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) p[q] = 0.0;
    if (flags & FD_EXPO) {
        const double xa = FD(x_a), xd = FD(x_d);
        const int xr = FD(x_reg), off0 = FD(coeff_off0), off1 = FD(coeff_off1);
        double x[PPL];
#pragma unroll
        for (int q = 0; q < PPL; ++q) x[q] = fma(xd, reg[q][xr], xa);
        if (flags & FD_STATE_EXPO) {
            // exposure of the exercise product: the coefficient row of the lane's state (product.py:150-184)
            double p0[PPL], p1[PPL];
#pragma unroll
            for (int q = 0; q < PPL; ++q) { p0[q] = 0.0; p1[q] = 0.0; }
            lean_poly_add<PPL>(a.coeffs + off0, a.n_basis, x, p0);
            lean_poly_add<PPL>(a.coeffs + off0 + a.n_basis, a.n_basis, x, p1);
#pragma unroll
            for (int q = 0; q < PPL; ++q) p[q] = est[q] > 0 ? p1[q] : p0[q];
        } else {
            if (off0 >= 0) lean_poly_add<PPL>(a.coeffs + off0, a.n_basis, x, p);
            if (off1 >= 0) lean_poly_add<PPL>(a.coeffs + off1, a.n_basis, x, p);
        }
    }
    // survival probability over the next interval, conditional on the credit state (cva_metric.py:66-89)
    auto cond_surv = [&](double (&cs)[PPL]) {
        const double ca = FD(c_a), cb = FD(c_b);
#pragma unroll
        for (int q = 0; q < PPL; ++q) cs[q] = ca;
        if (cb != 0.0) {
            const double cc0 = FD(c_c0), cc1 = FD(c_c1);
            const int cr = FD(c_reg);
#pragma unroll
            for (int q = 0; q < PPL; ++q) cs[q] = fma(cb, mcx_exp_tab(fma(cc1, reg[q][cr], cc0), etab, ec), ca);
        }
    };
    if (merged) {
        const double mb = FD(m_b), mc0 = FD(m_c0), mn1 = FD(m_n1), ms1 = FD(m_s1);
        const int nr = FD(ni_reg), sr = FD(s_reg);
        double w[PPL], cs[PPL];
#pragma unroll
        for (int q = 0; q < PPL; ++q) w[q] = mb * mcx_exp_tab(fma(ms1, reg[q][sr], fma(mn1, reg[q][nr], mc0)), etab, ec);
        cond_surv(cs);
#pragma unroll
        for (int q = 0; q < PPL; ++q) cva[q] = fma(fmax(p[q], 0.0), w[q] * (1.0 - cs[q]), cva[q]);
        return;
    }
    double e[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) e[q] = p[q] * inv[q];
    if (a.expo) {
        const int row = ldk(a.date_row + t);
        if (row >= 0) {
#pragma unroll
            for (int q = 0; q < PPL; ++q) if (live[q]) a.expo[(int64_t)row * a.ld_out + i[q]] = e[q];
        }
    }
    if (flags & FD_METRIC) {
        const double thr = FD(thr);
        double u[PPL];
#pragma unroll
        for (int q = 0; q < PPL; ++q) u[q] = dev_thr(e[q], thr);
        if (flags & FD_PROFILE) {
            const int rp = FD(rec_profile);
            double up[PPL], un[PPL];
#pragma unroll
            for (int q = 0; q < PPL; ++q) { up[q] = fmax(u[q], 0.0); un[q] = fmin(u[q], 0.0); }
            lean_record<PPL>(up, live, rp, a.n_rec, first_tile, lds);
            lean_record<PPL>(un, live, rp + 1, a.n_rec, first_tile, lds);
        }
        if (flags & FD_CVA) {
            const double sb = FD(s_b), sc0 = FD(s_c0), sc1 = FD(s_c1);
            const int sr = FD(s_reg);
            double sp[PPL], cs[PPL];
#pragma unroll
            for (int q = 0; q < PPL; ++q) sp[q] = sb * mcx_exp_tab(fma(sc1, reg[q][sr], sc0), etab, ec);
            cond_surv(cs);
#pragma unroll
            for (int q = 0; q < PPL; ++q) cva[q] = fma(fmax(u[q], 0.0), sp[q] * (1.0 - cs[q]), cva[q]);
        }
    }
}

#undef FD

// kf_lean.hip: launches the straight-line one-launch kernel for a book whose every date has a FastDate record; returns the
// grid size (= number of per-block partial records written to a.partials), or -1 when (slots, z) has no instantiation;
// simulate = false: the date programs run on the paths tensor a.k1.paths (the evaluation pass of mcx_fused_eval_paths);
// a.cva_dates != nullptr (simulating, no injected draws, no path / cashflow / exposure output): the cva-date kernel
int mcx_launch_kf_lean(const FusedArgs& a, const mcx_sim_desc& sd, int n_cu, bool inject, bool simulate, hipStream_t s);
