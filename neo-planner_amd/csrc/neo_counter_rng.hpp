// neo_counter_rng.hpp -- the counter-based jitter of the plan retries and the fleet's re-targeting: a normal draw is a
// pure function of (seed, id, a, b, domain, index), so a request draws the same alone and in any batch, on the host
// and on the device, without a generator object, a loop or a copy.
//
//   philox4x32_10      the block function (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
//                      SC'11; Random123): 4 x 32-bit counter, 2 x 32-bit key, ten rounds
//   counter_uniform    two output words -> u strictly inside (0, 1), 52 bits, every step exact
//   counter_log        ln x for a positive normal x from the bits and + - * / only
//   counter_probit     Phi^-1(u), Wichura's AS241 PPND16 (Applied Statistics 37 (3), 1988), Horner as CPython's
//                      statistics.py writes it
//   counter_normal     value e of the stream (seed, id, a, b, domain)
//
// neo_planner_amd/counter_rng.py is the NumPy model of this file: the same operations in the same order, every one
// rounded on its own (contraction is off in every function here; a host compiler that is not clang takes
// -ffp-contract=off on its command line).  Header and model agree bit for bit.  The fp64 division and square root are
// the correctly rounded ones, on the host and on gfx950.  Plain C++ as well as HIP: the harness
// tests/host_harness/counter_rng_host.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>

#if defined(__HIPCC__)
#define NEO_RNG_HD __host__ __device__ __forceinline__
#else
#define NEO_RNG_HD inline
#endif
#if defined(__clang__)
#define NEO_RNG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NEO_RNG_NO_CONTRACT
#endif

namespace neo {

constexpr uint32_t kRngDomainRetry = 1;   // BatchPlanner.plan's retry noise: a = attempt, b = 0
constexpr uint32_t kRngDomainTarget = 2;  // the fleet's target jitter: a = tick, b = target

struct Philox4 {
  uint32_t w[4];
};

NEO_RNG_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

// u = (((wa >> 6) * 2^26 + (wb >> 6)) + 0.5) * 2^-52: the integer is below 2^52, the sum below 2^53, the scale a power of two
NEO_RNG_HD double counter_uniform(uint32_t wa, uint32_t wb) {
  NEO_RNG_NO_CONTRACT
  const uint64_t k = ((uint64_t)(wa >> 6) << 26) | (uint64_t)(wb >> 6);
  return ((double)k + 0.5) * 2.220446049250313e-16;  // 2^-52
}

NEO_RNG_HD uint64_t counter_bits(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof b);
  return b;
}
NEO_RNG_HD double counter_from_bits(uint64_t b) {
  double x;
  memcpy(&x, &b, sizeof x);
  return x;
}

// ln x, x positive and normal: x = m 2^e with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), t = s^2,
// ln x = e ln2 + 2 s (1 + t / 3 + ... + t^11 / 23); |s| < 0.1716, so the first term left out is below 2e-20.  ln2 in two
// parts (the high one has 32 trailing zero bits: e * ln2_hi is exact).
NEO_RNG_HD double counter_log(double x) {
  NEO_RNG_NO_CONTRACT
  const uint64_t bits = counter_bits(x);
  const uint64_t mant = bits & 0x000FFFFFFFFFFFFFull;
  int e = (int)(bits >> 52) - 1023;
  uint64_t ex = 1023;
  if (mant >= 0x6A09E667F3BCDull) {  // m >= sqrt(2) (its mantissa, rounded up): halve it
    ex = 1022;
    e += 1;
  }
  const double m = counter_from_bits((ex << 52) | mant);
  const double s = (m - 1.0) / (m + 1.0);
  const double t = s * s;
  double p = 1.0 / 23.0;
  p = p * t + 1.0 / 21.0;
  p = p * t + 1.0 / 19.0;
  p = p * t + 1.0 / 17.0;
  p = p * t + 1.0 / 15.0;
  p = p * t + 1.0 / 13.0;
  p = p * t + 1.0 / 11.0;
  p = p * t + 1.0 / 9.0;
  p = p * t + 1.0 / 7.0;
  p = p * t + 1.0 / 5.0;
  p = p * t + 1.0 / 3.0;
  p = p * t + 1.0;
  const double de = (double)e;
  const double lo = (2.0 * s) * p + de * 1.90821492927058770002e-10;
  return de * 6.93147180369123816490e-01 + lo;
}

// Phi^-1(u), 0 < u < 1
NEO_RNG_HD double counter_probit(double u) {
  NEO_RNG_NO_CONTRACT
  const double q = u - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                            4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                          1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                            2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                          4.2313330701600911252e+1) * r + 1.0);
    return num / den;
  }
  double r = q <= 0.0 ? u : 1.0 - u;
  r = sqrt(-counter_log(r));
  double num, den;
  if (r <= 5.0) {
    r = r - 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
               1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
             4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
             2.05319162663775882187e+0) * r + 1.0);
  } else {
    r = r - 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
             5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
             5.99832206555887937690e-1) * r + 1.0);
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// value `half` (0: words 0 and 1, 1: words 2 and 3) of a block as a unit normal
NEO_RNG_HD double counter_block_normal(const Philox4 &o, int half) {
  return counter_probit(half ? counter_uniform(o.w[2], o.w[3]) : counter_uniform(o.w[0], o.w[1]));
}

// the block of values 2 j and 2 j + 1 of the stream: key (seed's low word, seed's high word), counter
// (id, a, b, domain << 24 | j); j < 2^24
NEO_RNG_HD Philox4 counter_stream_block(uint64_t seed, uint32_t id, uint32_t a, uint32_t b, uint32_t domain, uint32_t j) {
  return philox4x32_10(id, a, b, (domain << 24) | j, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// value e of the stream: a unit normal
NEO_RNG_HD double counter_normal(uint64_t seed, uint32_t id, uint32_t a, uint32_t b, uint32_t domain, uint32_t e) {
  return counter_block_normal(counter_stream_block(seed, id, a, b, domain, e >> 1), (int)(e & 1u));
}

}  // namespace neo
