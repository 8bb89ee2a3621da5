// mcx_dual_step.h — the dual (forward-mode) step maps of the one-factor model kinds: step_slot (mcx_device.h) in dual numbers with
// MCX_TANGENT_NP tangents, ONE copy for the narrow dual path kernels (kt_book.hip kt_paths / kt_paths_chol) and the wide one
// (kt_wide.hip kt_paths_wide), as step_slot is one copy for k1_paths and k1_paths_wide.
//
// What differs between the callers is where a slot's numbers live, and the maps read them through a loader: ld(j) is the dual number
// whose value is entry j of a table and whose tangents are row j of the table's derivative rows [.][NP] (always a wave-uniform
// device table: scalar loads at the point of use).
//   DualKarg  : the value table sits in the kernel-argument segment (the slot parameters of a narrow sim, K1Args::slots[s].p);
//   DualTable : the value table is a device table too (the aux rows everywhere; the slot parameters of a wide sim).
// A correction to a map (a clamp convention, an operand order) is made here and reaches every kernel.
#pragma once
#include "mcx_dual.h"

constexpr int NP = MCX_TANGENT_NP;
typedef Dual<NP> DN;

__device__ __forceinline__ DN ld_dual(double v, const double* __restrict__ d)      // wave-uniform derivative row -> scalar loads
{
    DN r;
    r.v = v;
#pragma unroll
    for (int q = 0; q < NP; ++q) r.d[q] = ldk(d + q);
    return r;
}

// acc + l z for a dual factor entry and a plain normal: every image is one multiply-add, as the primal product's (k1_paths.hip)
__device__ __forceinline__ DN ktp_fma(const DN& l, double z, const DN& acc)
{
    DN r;
    r.v = fma(l.v, z, acc.v);
#pragma unroll
    for (int q = 0; q < NP; ++q) r.d[q] = fma(l.d[q], z, acc.d[q]);
    return r;
}

struct DualKarg {
    const double* __restrict__ v;
    const double* __restrict__ d;
    __device__ __forceinline__ DN operator()(int j) const { return ld_dual(v[j], d + j * NP); }
};
struct DualTable {
    const double* __restrict__ v;
    const double* __restrict__ d;
    __device__ __forceinline__ DN operator()(int j) const { return ld_dual(ldk(v + j), d + j * NP); }
};

// One EULER sub-step of a slot of `kind` (wave-uniform): p its parameters, ax its aux row of the step, zs its correlated normal (a
// plain double: the correlations are not model parameters).  HW: also the Hull-White step, which only kt_paths_wide<., true> has;
// the entry points refuse every kind without a case here.
template <bool HW, class P>
__device__ __forceinline__ void dual_step_euler(int kind, const P& p, const DualTable& ax, double dt, double sq, double zs, DN& s0, DN& s1)
{
    switch (kind) {
    case MCX_MODEL_BS: {                                          // black_scholes.py:79-85
        const DN sigma = p(1), rate = p(2);
        s0 = s0 + (rate * s0 * dt + sigma * s0 * (sq * zs));
        break;
    }
    case MCX_MODEL_VASICEK: {                                     // vasicek.py:88-112
        const DN sigma = p(1), mean = p(2), speed = p(3);
        const DN r = s0;
        s1 = s1 + r * dt;
        s0 = r + speed * (mean - r) * dt + sigma * (sq * zs);
        break;
    }
    case MCX_MODEL_CIRPP: {                                       // cirpp.py:188-198
        const DN kappa = p(0), theta = p(1), sigma = p(2);
        const DN psi = ax(0);
        const DN y = s0;
        const DN sy = dsqrt(dclamp_min(y, 0.0));
        const DN yn = y + kappa * (theta - y) * dt + sigma * sy * (sq * zs);
        s1 = s1 + (y + psi) * dt;
        s0 = dclamp_min(yn, 1e-12);
        break;
    }
    case MCX_MODEL_CIRPP_DET: {                                   // cirpp.py:155-172
        s1 = s1 + ax(0) * dt;
        s0 = ax(1);
        break;
    }
    default:
        if (HW && kind == MCX_MODEL_HW) {                         // mcx_device.h case MCX_MODEL_HW in dual numbers; theta_k = aux[0]
            const DN sigma = p(1), speed = p(3);
            const DN theta = ax(0);
            const DN r = s0;
            s1 = s1 + r * dt;
            s0 = r + (theta - speed * r) * dt + sigma * (sq * zs);
        }
        break;
    }
}

// One ANALYTICAL sub-step: the primal analytic branches of step_slot in dual numbers.  zs = (L z)_slot is a dual number, the factor
// of the per-dt covariance depends on the parameters.  Two details of the signature are there for kt_paths_wide's code alone (device
// assembly compared per kernel with the restated maps it replaced, profiles/dual_step_asm_compare.md; kt_book.hip's kernels are
// indifferent to both):
//   * bs is kind == MCX_MODEL_BS as the caller computed it before its step loop.  Testing the kind again in here cost the two
//     HW = true instantiations one v_cmp + v_cndmask and moved their allocation (71 -> 72 VGPRs, SGPR spills 69 -> 65 and 4 -> 0);
//   * zs travels by value.  By reference, kt_paths_wide<true, false> came out with the same instructions in another order.
template <bool HW, class P>
__device__ __forceinline__ void dual_step_analytical(bool bs, int kind, const P& p, const DualTable& ax, double dt, const DN zs, DN& s0, DN& s1)
{
    if (bs) {                                                     // black_scholes.py:61-67
        const DN drift = ax(0), ito = ax(1);
        s0 = s0 * dexp(drift + (zs - ito));
    } else if (HW && kind == MCX_MODEL_HW) {                      // r' = r E + shift + w, hull_white.py _step_aux
        const DN decay = ax(0), shift = ax(1);
        const DN r = s0;
        s1 = s1 + r * dt;
        s0 = (r * decay + shift) + zs;
    } else {                                                      // MCX_MODEL_VASICEK, vasicek.py:76-86
        const DN mean = p(2), decay = ax(0);
        const DN r = s0;
        s1 = s1 + r * dt;
        s0 = (mean + (r - mean) * decay) + zs;
    }
}
