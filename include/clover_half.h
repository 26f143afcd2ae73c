/*
 * clover_half.h -- IEEE binary16 <-> fp32 on the host in integer arithmetic, for the element accessors and the scalar twins of
 * CloverVector16 / CloverMatrix16: what _mm_cvtss_sh / _mm_cvtsh_ss (round to nearest even, subnormals kept) compute, without
 * requiring F16C on the build machine.
 */
#ifndef CLOVER_HALF_H
#define CLOVER_HALF_H

#include <stdint.h>
#include <string.h>

namespace clover_hip {
namespace half {

inline float to_f32(uint16_t h)
{
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 31u, m = h & 0x3FFu, u;
    if (e == 31u) u = s | 0x7F800000u | (m << 13);                   /* inf, NaN */
    else if (e == 0u) {
        if (m == 0u) u = s;
        else {                                                       /* subnormal: m * 2^-24 */
            e = 113u;
            while (!(m & 0x400u)) { m <<= 1; e--; }
            u = s | (e << 23) | ((m & 0x3FFu) << 13);
        }
    } else u = s | ((e + 112u) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

inline uint16_t from_f32(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t s = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t e = (u >> 23) & 0xFFu, m = u & 0x7FFFFFu;
    if (e == 0xFFu) return (uint16_t)(s | 0x7C00u | (m ? (0x200u | (m >> 13)) : 0u));
    if (e == 0u) return s;
    if (e >= 143u) return (uint16_t)(s | 0x7C00u);                   /* 2^16 and beyond */
    const uint32_t sig = 0x800000u | m;                              /* value = sig * 2^(e - 150) */
    const uint32_t drop = e >= 113u ? 13u : 126u - e;                /* normal: 11 significant bits; below 2^-14: units of 2^-24 */
    if (drop >= 25u) return s;
    uint32_t q = sig >> drop;
    const uint32_t rem = sig & ((1u << drop) - 1u), half_ulp = 1u << (drop - 1u);
    if (rem > half_ulp || (rem == half_ulp && (q & 1u))) q++;        /* nearest, ties to even; a carry moves into the exponent */
    return (uint16_t)(s | (e >= 113u ? ((e - 113u) << 10) + q : q));
}

}  // namespace half
}  // namespace clover_hip

#endif
