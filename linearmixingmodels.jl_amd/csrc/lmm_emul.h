// lmm_emul.h -- exact int8 modular emulation of a Float64 product C -= A B' (DESIGN.md 4.17): constants and the scalar steps (row
// scaling, residues, CRT reconstruction) shared by the device kernels (lmm_kernels_i8.hip) and the host-only test entry
// lmm_dev_emul_host (lmm_api.hip), so that the CPU test checks the very code the GPU runs.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LMM_HD __host__ __device__
#else
#define LMM_HD
#endif

#define LMM_EMUL_MAXMOD 16
#define LMM_EMUL_MINMOD 8
#define LMM_EMUL_MAXBITS 58      // |a'| <= 2^58: emul_residue's three limbs stay below 2^29

// The 16 largest pairwise-coprime integers <= 256; the first nmod of them are used.
static const int kEmulModuli[LMM_EMUL_MAXMOD] = {256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193};

// By-value kernel argument.  w_t = (P / p_t) ((P / p_t)^-1 mod p_t) < P; every w_t and P itself are cut at bits 85 and 44 into three
// doubles (41 + 41 + 44 bits, each exact).
struct EmulConst {
  int nmod;
  int p[LMM_EMUL_MAXMOD];
  int c1[LMM_EMUL_MAXMOD], c2[LMM_EMUL_MAXMOD];      // 2^20 mod p, 2^40 mod p (emul_residue)
  double w1[LMM_EMUL_MAXMOD], w2[LMM_EMUL_MAXMOD], w3[LMM_EMUL_MAXMOD];
  double P1, P2, P3, Pinv, Phalf;
};

typedef unsigned __int128 emul_u128;

inline emul_u128 emul_modulus_product(int nmod) {
  emul_u128 P = 1;
  for (int t = 0; t < nmod; ++t) P *= (emul_u128)kEmulModuli[t];
  return P;
}
inline void emul_split3(emul_u128 v, double& a, double& b, double& c) {
  a = std::ldexp((double)(uint64_t)(v >> 85), 85);
  b = std::ldexp((double)(uint64_t)((v >> 44) & ((uint64_t(1) << 41) - 1)), 44);
  c = (double)(uint64_t)(v & ((uint64_t(1) << 44) - 1));
}
inline EmulConst emul_make_const(int nmod) {
  EmulConst c{};
  c.nmod = nmod;
  const emul_u128 P = emul_modulus_product(nmod);
  emul_split3(P, c.P1, c.P2, c.P3);
  c.Pinv = 1.0 / ((c.P1 + c.P2) + c.P3);
  c.Phalf = 0.5 * ((c.P1 + c.P2) + c.P3);
  for (int t = 0; t < nmod; ++t) {
    const int p = kEmulModuli[t];
    c.p[t] = p;
    c.c1[t] = (int)((uint64_t(1) << 20) % p);
    c.c2[t] = (int)((uint64_t(1) << 40) % p);
    const emul_u128 Mt = P / (emul_u128)p;
    const int r = (int)(Mt % (emul_u128)p);
    int inv = 1;
    while ((r * inv) % p != 1) ++inv;
    emul_split3(Mt * (emul_u128)inv, c.w1[t], c.w2[t], c.w3[t]);
  }
  return c;
}
// Largest b <= LMM_EMUL_MAXBITS with K 2^(2b) < P / 2: a depth-K dot product of integers |a'| <= 2^b is determined by its residues.
inline int emul_bits(int nmod, long long K) {
  const emul_u128 half = emul_modulus_product(nmod) / 2;
  int b = LMM_EMUL_MAXBITS;
  while (b > 0 && (emul_u128)K > ((half - 1) >> (2 * b))) --b;      // K 2^(2b) <= half - 1, without overflowing 128 bits
  return b;
}

// ceil(log2 amax) for a finite amax > 0
LMM_HD inline int emul_row_exp(double amax) {
  int q;
  const double f = frexp(amax, &q);
  return f == 0.5 ? q - 1 : q;
}
// a' = trunc(a 2^sh), sh = b - e_row: an exact power-of-two scaling, |a'| <= 2^b
LMM_HD inline long long emul_trunc(double a, int sh) { return (long long)ldexp(a, sh); }
// v mod p in the symmetric range ([-128, 127] for p = 256; +128 is returned as 128 and wraps to -128 in the int8 store)
LMM_HD inline int emul_mod_sym(int x, int p, float rp) {
  // |x| < 2^29: the float quotient is off by less than 0.5, so one correction each way lands in [lo, lo + p - 1]
#if defined(__HIP_DEVICE_COMPILE__)
  const int q = __float2int_rn((float)x * rp);
#else
  const int q = (int)lrintf((float)x * rp);
#endif
  const int lo = -(p / 2);
  int r = x - q * p;
  r += (r < lo) ? p : 0;
  r -= (r > lo + p - 1) ? p : 0;
  return r;
}
LMM_HD inline int emul_residue(long long v, int p, float rp, int c1, int c2) {
  const bool neg = v < 0;
  const unsigned long long m = neg ? (unsigned long long)(-v) : (unsigned long long)v;
  const int x = (int)(m & 0xFFFFF) + (int)((m >> 20) & 0xFFFFF) * c1 + (int)(m >> 40) * c2;
  const int r = emul_mod_sym(x, p, rp);
  return neg ? -r : r;
}
// The integer X, |X| < P / 2, with X = u_t mod p_t for all t, rounded once to Float64.  S1 and S2 are exact (41-bit chunks, 8-bit
// residues, 16 terms); S1 - q P1 and S2 - q P2 are exact; their sum rounds X to 53 bits; the third term is below one ulp of P.
LMM_HD inline double emul_crt_at(double S1, double S2, double S3, double q, const EmulConst& c) {
  return ((S1 - q * c.P1) + (S2 - q * c.P2)) + (S3 - q * c.P3);
}
LMM_HD inline double emul_crt(const int* u, const EmulConst& c) {
  double S1 = 0.0, S2 = 0.0, S3 = 0.0;
#pragma unroll
  for (int t = 0; t < LMM_EMUL_MAXMOD; ++t)
    if (t < c.nmod) {
      const double ut = (double)u[t];
      S1 += ut * c.w1[t];
      S2 += ut * c.w2[t];
      S3 += ut * c.w3[t];
    }
  double q = rint((S1 + S2) * c.Pinv);
  double X = emul_crt_at(S1, S2, S3, q, c);
  if (X > c.Phalf) X = emul_crt_at(S1, S2, S3, q + 1.0, c);
  else if (X < -c.Phalf) X = emul_crt_at(S1, S2, S3, q - 1.0, c);
  return X;
}
