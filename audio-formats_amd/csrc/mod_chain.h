// mod_chain.h -- the two pieces of float arithmetic of the MOD mixer that the host control layer and the device mixer
// must agree on bit for bit (pocketmod.d:664-721): the x86-64 float-to-int conversion and the position chain
// `position += increment` jumped k steps ahead in closed form.  Header-only, host and device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AFG_MOD_HD __host__ __device__ inline
#else
#define AFG_MOD_HD inline
#endif

namespace afg_mod {

// D's cast(int) of a float as x86-64 executes it (cvttss2si): truncation toward zero, and INT_MIN ("integer indefinite")
// for NaN and for anything outside [-2^31, 2^31).  A plain static_cast<int> of such a value is undefined behaviour in C++,
// and the device's v_cvt_i32_f32 saturates instead; both sides go through this helper.
AFG_MOD_HD int32_t cvt_i32(float x)
{
    if (!(x > -2147483904.0f && x < 2147483648.0f)) return INT32_MIN;     // NaN, infinities, out of range
    return (int32_t)x;                                                      // (x > -2^31 - 256: the next float down is -2^31 - 256)
}

AFG_MOD_HD uint32_t f2u(float x) { union { float f; uint32_t u; } v; v.f = x; return v.u; }
AFG_MOD_HD float u2f(uint32_t x) { union { float f; uint32_t u; } v; v.u = x; return v.f; }

// p after k sequential float32 adds p = p + inc, without k adds.
//
// Let p lie in the binade [2^e, 2^(e+1)) with ulp u = 2^(e-23), p = a * u with a an integer in [2^23, 2^24).  While the
// exact sum p + inc stays below 2^(e+1), fl(p + inc) = (a + RN(q)) * u with q = inc / u (exact: u is a power of two) and
// the rounding to nearest even taken on a + RN(q).  Away from ties that is a constant step d = RN(q): the chain is
// a_k = a_0 + k * d inside the binade, and it stalls (d = 0) where the reference's position stalls.  On a tie (q = m + 1/2)
// the first step lands on an even mantissa and every later one adds the even one of m and m + 1: a constant step again.
// The step that leaves the binade, a step from 0 or from a subnormal, and the first step of a tie from an odd mantissa
// are real float adds.  Exact for any finite inc >= 0 and p >= 0 (the mixer's chains: pocketmod.d:687 emits no frame
// for other increments).
AFG_MOD_HD float chain_jump(float p, float inc, uint32_t k)
{
    while (k) {
        const uint32_t bits = f2u(p);
        const uint32_t ex = (bits >> 23) & 0xffu;
        if (!(p > 0.0f) || ex == 0 || ex >= 0xfeu || !(inc >= 0.0f)) { p = p + inc; k--; continue; }
        const int64_t a = (int64_t)((bits & 0x7fffffu) | 0x800000u);
        // q = inc / u = inc * 2^(150 - ex): exact while the scaled value stays normal; a q of 2^24 or more always leaves
        // the binade, so the scale is capped there (and the sum test below takes the real add)
        const int sh = 150 - (int)ex;                                   // u = 2^(ex - 150)
        const uint32_t ib = f2u(inc);
        const int iex = (int)((ib >> 23) & 0xffu);
        if (iex == 0) {                                                 // inc is 0 or subnormal: far below u
            if (inc == 0.0f) return p;                                  // x + 0 = x
            p = p + inc; k--; continue;
        }
        if (iex + sh >= 127 + 25) { p = p + inc; k--; continue; }       // q >= 2^25: leaves the binade
        if (iex + sh <= 127 - 2) return p;                              // q < 1/2 (not a tie): every step rounds back to p
        const float q = u2f((ib & 0x807fffffu) | ((uint32_t)(iex + sh) << 23));
        const int64_t m = (int64_t)q;                                   // floor: q > 0
        const float fr = q - (float)m;                                  // exact
        if ((int64_t)a + m + (fr > 0.0f ? 1 : 0) > (int64_t)0xffffff) { p = p + inc; k--; continue; }   // a + q >= 2^24
        int64_t d;
        if (fr == 0.5f) {
            if (a & 1) { p = p + inc; k--; continue; }                  // lands on the even neighbour; constant from there
            d = m + (m & 1);
        } else {
            d = fr > 0.5f ? m + 1 : m;
        }
        if (d == 0) return p;
        // step j (from a + j*d) stays in the binade while a + j*d + q < 2^24, i.e. j*d <= 2^24 - a - m - 1
        const int64_t room = (int64_t)0x1000000 - a - m - 1;
        int64_t s = (int64_t)k;
        if ((s - 1) * d > room) s = (int64_t)((uint32_t)room / (uint32_t)d) + 1;       // (room < 2^24, d < 2^25: 32 bits)
        const int64_t a1 = a + s * d;                                   // <= 2^24: representable
        p = u2f(f2u((float)a1) - ((uint32_t)sh << 23));                 // a1 * u (a1 = 2^24 lands on the next binade's start)
        k -= (uint32_t)s;
    }
    return p;
}

}  // namespace afg_mod
