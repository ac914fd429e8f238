// sha256_experiments.h — superseded forms of the SHA-256 rounds, kept for the microbenchmarks
// that compare them with what the kernels run (skew.hip, oct.hip). The library includes none of
// this; the product forms are in bs_amd/csrc/sha256_device.h.
#pragma once
#include "../../bs_amd/csrc/sha256_device.h"

namespace bsg {

// SHA_ROUND in plain C operators, left to hipcc's selection.
#define SHA_ROUND_C(a, b, c, d, e, f, g, h, kw)                               \
  do {                                                                         \
    const uint32_t s1_ = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);               \
    const uint32_t ch_ = (e & f) | (~e & g);                                   \
    const uint32_t t1_ = (h + (kw)) + s1_ + ch_;                               \
    d += t1_;                                                                  \
    const uint32_t s0_ = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);               \
    const uint32_t mj_ = (a & b) | (c & (a | b));                              \
    h = t1_ + s0_ + mj_;                                                       \
  } while (0)

// Rounds only, with K[t] + W[t] precomputed elsewhere (long-chain path experiments).
template <bool ASM>
__device__ __forceinline__ void sha256_rounds_kw(uint32_t (&st)[8], const uint32_t (&KW)[64]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6],
           h = st[7];
#pragma unroll
  for (int t = 0; t < 64; t += 8) {
#define R_(...) do { if (ASM) SHA_ROUND(__VA_ARGS__); else SHA_ROUND_C(__VA_ARGS__); } while (0)
    R_(a, b, c, d, e, f, g, h, KW[t + 0]);
    R_(h, a, b, c, d, e, f, g, KW[t + 1]);
    R_(g, h, a, b, c, d, e, f, KW[t + 2]);
    R_(f, g, h, a, b, c, d, e, KW[t + 3]);
    R_(e, f, g, h, a, b, c, d, KW[t + 4]);
    R_(d, e, f, g, h, a, b, c, KW[t + 5]);
    R_(c, d, e, f, g, h, a, b, KW[t + 6]);
    R_(b, c, d, e, f, g, h, a, KW[t + 7]);
#undef R_
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
  st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// ---------------------------------------------------------------------------------------------
// Banked lane pair for one long chain (wave mode, round 2; superseded by the skewed pair). A
// single chain is bound by one wave's issue rate (~4.5 cycles per instruction, dependent or not;
// an s_nop wait state costs the same), so what counts is instructions per round. The round is
// split over two lanes that run the same 10 instructions (14 for the whole round in one lane),
// the E lane holding (e,f,g,h) and the A lane (a,b,c,d):
//   S = Sigma(R1): 3 x v_alignbit with per-lane counts + xor3      E: Sigma1(e)     A: Sigma0(a)
//   x = R1 ^ (R3 & xm)          (xm = 0 on E, ~0 on A)             E: e             A: a^c
//   F = Ch(x, R2, R3)                                               E: Ch(e,f,g)     A: Maj(a,b,c)
//   U = S + F + Q                                                   E: T1 + d = e'   A: T2 - d
//   n = U + U(lane-1), written on A lanes only (DPP bank mask)     E: e'            A: T1 + T2 = a'
// with Q prepared during the previous round (in the DPP hazard shadow of U):
//   P = (R4 ^ xm) + kwl         (kwl = K+W on E, 1 on A)           E: h + KW        A: -d
//   Q = P + R4(lane+1), written on E lanes only                     E: h + KW + d    A: -d
// DPP bank masks pick lanes in groups of 4 (bank k of a 16-lane row = lanes 4k..4k+3), so the
// pair is (lane 3, lane 4) of every 8: E lanes are those with lane & 4 == 0. The other lanes
// compute garbage and are ignored. kwl comes from a per-lane LDS row (E lanes: the block's K+W
// row; A lanes: a row of ones).
struct BankLane {
  uint32_t rot1, rot2, rot3, xm;
  bool a_side;
};

__device__ __forceinline__ BankLane bank_lane() {
  BankLane b;
  b.a_side = (threadIdx.x & 4u) != 0u;
  b.rot1 = b.a_side ? 2u : 6u;
  b.rot2 = b.a_side ? 13u : 11u;
  b.rot3 = b.a_side ? 22u : 25u;
  b.xm = b.a_side ? 0xffffffffu : 0u;
  return b;
}
constexpr uint32_t kBankE = 3, kBankA = 4;  // the lanes holding (e,f,g,h) and (a,b,c,d)

// One round, hand-scheduled in one asm block (the compiler's own schedule left the DPP
// source hazards to s_nop). q in: this round's Q; out: the next round's (from kwn).
__device__ __forceinline__ void bank_round(uint32_t& r1, uint32_t& r2, uint32_t& r3,
                                           uint32_t& r4, uint32_t& q, uint32_t kwn,
                                           const BankLane& b) {
  uint32_t u, qn, t0, t1, t2, x;
  asm("v_alignbit_b32 %[t0], %[r1], %[r1], %[s1]\n\t"
      "v_alignbit_b32 %[t1], %[r1], %[r1], %[s2]\n\t"
      "v_alignbit_b32 %[t2], %[r1], %[r1], %[s3]\n\t"
      "v_bitop3_b32 %[x], %[r1], %[r3], %[xm] bitop3:0x78\n\t"
      "v_bitop3_b32 %[t0], %[t0], %[t1], %[t2] bitop3:0x96\n\t"
      "v_bitop3_b32 %[x], %[x], %[r2], %[r3] bitop3:0xca\n\t"
      "v_add3_u32 %[u], %[t0], %[x], %[q]\n\t"
      "v_xad_u32 %[qn], %[r3], %[xm], %[kwn]\n\t"
      "v_add_u32_dpp %[qn], %[r3], %[qn] row_shl:1 row_mask:0xf bank_mask:0x5\n\t"
      "v_add_u32_dpp %[u], %[u], %[u] row_shr:1 row_mask:0xf bank_mask:0xa"
      : [u] "=&v"(u), [qn] "=&v"(qn), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
        [x] "=&v"(x)
      : [r1] "v"(r1), [r2] "v"(r2), [r3] "v"(r3), [q] "v"(q), [kwn] "v"(kwn),
        [s1] "v"(b.rot1), [s2] "v"(b.rot2), [s3] "v"(b.rot3), [xm] "v"(b.xm));
  r4 = r3;
  r3 = r2;
  r2 = r1;
  r1 = u;
  q = qn;
}

// Q of round 0 of a block, from the block's starting state.
__device__ __forceinline__ uint32_t bank_q0(uint32_t r4, uint32_t kw0, const BankLane& b) {
  uint32_t q;
  asm("v_xad_u32 %[q], %[r4], %[xm], %[kw]\n\t"
      "s_nop 1\n\t"
      "v_add_u32_dpp %[q], %[r4], %[q] row_shl:1 row_mask:0xf bank_mask:0x5"
      : [q] "=&v"(q)
      : [r4] "v"(r4), [xm] "v"(b.xm), [kw] "v"(kw0));
  return q;
}

// 64 rounds on this lane's half state s[4] (E: H4..H7, A: H0..H3) from this lane's LDS row
// (16 x 16 B); adds the block result into s if `active` (lanes of finished chains keep theirs).
__device__ __forceinline__ void sha256_rounds_bank(uint32_t (&s)[4], const uint32_t* row,
                                                   const BankLane& b, bool active = true) {
  typedef uint32_t u32x4r __attribute__((ext_vector_type(4), aligned(16)));
  const u32x4r* r = reinterpret_cast<const u32x4r*>(row);
  uint32_t r1 = s[0], r2 = s[1], r3 = s[2], r4 = s[3];
  u32x4r kw = r[0];
  uint32_t q = bank_q0(r4, kw.x, b);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const u32x4r kn = r[i < 15 ? i + 1 : 15];
    bank_round(r1, r2, r3, r4, q, kw.y, b);
    bank_round(r1, r2, r3, r4, q, kw.z, b);
    bank_round(r1, r2, r3, r4, q, kw.w, b);
    bank_round(r1, r2, r3, r4, q, kn.x, b);  // after round 63 this Q is not used
    kw = kn;
  }
  // 64 rounds (a multiple of 4): the names are back in place, r1 = e|a ...
  s[0] = active ? s[0] + r1 : s[0];
  s[1] = active ? s[1] + r2 : s[1];
  s[2] = active ? s[2] + r3 : s[2];
  s[3] = active ? s[3] + r4 : s[3];
}

// ---------------------------------------------------------------------------------------------
// One block (64 rounds) of the skewed lane pair (SkewLane, sha256_device.h) on this lane's half
// state from its LDS row (E lanes: the block's 64 K+W words; A lanes: 64 ones), 16-byte
// aligned; feed-forward only if `active`. The 66 iterations are one generated asm statement
// (tools/gen_skew_asm.py documents the schedule): as separate asm blocks, each containing the
// DPP exchange, hipcc put an s_nop in front of every other one. The kernels run the block loop
// sha256_blocks_skew instead.
#include "sha256_skew_block.inc"
__device__ __forceinline__ void sha256_rounds_skew(uint32_t (&hs)[4], const uint32_t* row,
                                                   const SkewLane& b, bool active = true) {
  // slot s holds V(j), j = s (mod 4): V(-2) = H4|H2, V(-3) = H5|H3, V(-4) = H6|-, V(-5) = H7|H1
  uint32_t v2 = hs[2], v1 = hs[3], v0 = hs[0], v3 = hs[1];
  const uint32_t addr = (uint32_t)reinterpret_cast<uintptr_t>(
      (__attribute__((address_space(3))) const uint32_t*)row);
  const uint64_t amask = 0xAAAAAAAAAAAAAAAAull;  // A lanes: odd
  asm volatile(BSG_SKEW_BLOCK_ASM
               : [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3)
               : [row] "v"(addr), [xm] "v"(b.xm), [s1] "v"(b.rot1), [s2] "v"(b.rot2),
                 [s3] "v"(b.rot3), [amask] "s"(amask)
               : "memory", BSG_SKEW_BLOCK_CLOBBERS);
  if (active) {
    hs[0] += v0;  // A: a_64 -> H0 | E: e_62 -> H6
    hs[1] += v3;  // A: a_63 -> H1 | E: e_61 -> H7
    hs[2] += v2;  // A: a_62 -> H2 | E: e_64 -> H4
    hs[3] += v1;  // A: a_61 -> H3 | E: e_63 -> H5
  }
}

}  // namespace bsg
