// Any Life-like (outer-totalistic Moore) rule, K generations per sweep, bit-sliced: life_rule_bits.
//
// The rule is data: two 9-bit masks, birth[n] / survive[n] for n = 0..8 live neighbours (B36/S23,
// B3678/S34678, B2/S, ...; 2^18 rules). Conway's B3/S23 keeps its own kernels (stencil_life.hip);
// every other rule runs here, single steps included (life_wave / life_tb2 are SWAR compares of
// B3/S23 and cannot take a table).
//
// Division of work (life_bits', unchanged): one wave per task, no LDS, no barriers. A lane loads 32
// u8 cells of a row (two 16-B vectors) and packs them into one word (bit j = cell x + j, life_pack4);
// segments of 62 owned lanes (1,984 cells) overlap by one halo lane per side; the x neighbours come
// through DPP lane shifts and v_alignbit; K levels of streaming row state live in registers (per level
// the 3-sums of its last two input rows, the 2-sum and the cells of the last one: 7 words); the last
// level unpacks to bytes for the store. 1 B read + 1 B written per cell per K generations.
//
// What is new is the arithmetic of a generation (32 cells per lane at once):
//   row sums on arrival, each ONE three-input boolean op:  c0 = L ^ R, c1 = L & R (2-sum L + R),
//     s0 = L ^ X ^ R, s1 = maj(L, X, R) (3-sum)
//   the exact 4-bit neighbour count N = s(r-1) + s(r+1) + c(r), 0..8: two full adders (xor3 + maj3
//     each), a half adder, and n2 = k1a ^ k1b, n3 = k1a & k1b. life_bits keeps only n2 | n3; here both
//     are needed, and n3 set means exactly 8 (then n0 = n1 = n2 = 0).
//   the rule as a multiplexer tree over 18 leaves, next = self ? survive[N] : birth[N]:
//     9 selects on self (L[n] = self ? S[n] : B[n]), 4 on n0, 2 on n1, 1 on n2 and 1 on n3 that picks
//     the n = 8 leaf: 17 selects, each one (c & a) | (~c & b).
//   Leaves. The 18 table bits are expanded at kernel entry into 0 / ~0 words. A select between two
//   wave-uniform leaves would need two scalar operands, and a gfx950 VALU op reads one; so the leaves
//   live in 18 VGPRs for the whole sweep, and since they are per-lane anyway the held-cell mask is
//   folded into them (S[n] |= hm, B[n] &= ~hm: a held cell "survives" whatever its count and is never
//   born), which removes life_bits' closing select on hm. Cost: 18 VGPRs.
//
// VALU ops per generation of 32 cells, read off the gfx950 disassembly (an estimate from the code,
// not a measurement): 2 DPP moves + 2 v_alignbit + 4 row-sum ops (v_xor, v_and, v_xor, v_bfi), 7 for
// the count (4 v_bitop3 for the two full adders, v_xor for n1, and the compiler folds k1b away:
// n2 = bitop3(k1a ^ (z1 & k0)), n3 = bitop3(k1a & z1 & k0)), 17 selects (15 v_bfi + 2 v_bitop3) = 32,
// against life_bits' ~22: 1.45x the arithmetic.
//
// Exactness for every rule, B0 rules included. Nothing in life_bits' overlap argument uses the rule:
//   - x: a lane's word of generation t depends on its own and its neighbours' words of t - 1 only
//     through the cells x - 1 .. x + 32. The halo lanes (0, 63) see a wrong cell beyond the wave, so a
//     generation corrupts one more cell of them from the outside in; the owned lanes 1..62 read the
//     halo lanes' innermost cell, which is wrong only after 32 generations: K <= 32.
//   - rows: output row r needs rows r - K .. r + K of the input (halo >= K rows of valid ghosts); rows
//     clamped to the storage (lz < 0, lz >= lz_max) only prime the pipeline or lie outside the grid.
//   - what a B0 rule changes is that a cell can be born out of an all-dead neighbourhood, so dead
//     padding no longer stays dead by itself. It never had to: pad cells (x >= nx), the frame columns
//     and rows (x = 0, x = nx - 1, gz = 0, gz = gnz - 1) and rows outside the grid (gz < 0, gz > gnz - 1,
//     held by the row test of every level) are HELD, by the leaves' hm bits or by the wave-uniform row
//     test, whatever the rule says. A lane wholly outside the row (x < 0 or x >= pitch) does evolve
//     by the rule, on finite values read from the nearest in-row vector, but its only in-row
//     neighbour is cell x = 0 or a cell >= nx - 1 (pitch >= nx), which are held and therefore read no
//     neighbour; it is never stored (own is false). Levels that have not yet seen three valid rows
//     produce garbage (with B0, non-zero garbage), and that garbage only ever reaches rows before the
//     first row a level may emit: level l's first valid row is zs - K + l - 1, level K's is zs - 1,
//     and stores start at zs.
//
// Resources (scripts/kernel_resources.py; without / with the residual): VGPRs 48 / 54, 58 / 60,
// 64 / 70, 74 / 78, 90 / 94, 108 / 112, 144 / 146, 177 / 184 for K = 1, 2, 3, 4, 6, 8, 12, 16; no
// instance spills or uses scratch. Waves per SIMD: 8, 8, 8-7, 6, 5, 4, 3, 2.
//
// Measured on one MI355X, 32768^2, HighLife (B36/S23) against Conway's kernels at equal K,
// alternating in one process, best of 5 rounds of 100 sweeps, spread within 0.3 % (GCells/s;
// profiles/r08_life_rules/). Both move one byte in and one out per cell per sweep, so the ratio is
// the cost of the arithmetic alone:
//     K        1      2      3      4       6       8      12      16
//     Conway   2438   4842   6329   8310   12157   16280   22639   22286   (life_wave, life_tb2, life_bits)
//     here     2232   4415   6532   8584   12656   16217   19233   16380
//     ratio    0.92   0.91   1.03   1.03    1.04    1.00    0.85    0.73
// Up to K = 8 a sweep costs one pass over memory (1.00 .. 1.10 of this kernel's single step); K = 12
// is bound by the arithmetic (1.39) and is the fastest per generation, the default depth; K = 16
// (2 waves per SIMD) loses to it. The naive kernel runs the same rule at 474 GCells/s, so single
// steps and pairs run here too.
#include <algorithm>

#include "kcommon.hpp"
#include "launchers.hpp"
#include "life_pack.hpp"
#include "mdfx/kernels.hpp"

namespace mdfx {
namespace dev {

namespace {

// three-input boolean ops, one VALU instruction each. The select is v_bfi_b32 from the plain
// expression. A full adder's xor3 / maj3 pair came out of the plain expressions as 2 v_xor + v_xor +
// v_bfi (the compiler shares no xor between them); asking for v_bitop3_b32 by its truth table (bit
// index a << 2 | b << 1 | c) makes it one op each.
__device__ __forceinline__ uint32_t bsel(uint32_t c, uint32_t a, uint32_t b) { return (c & a) | (~c & b); }
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
}
#else
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }
#endif

// per-level streaming state: 3-sums of rows q-2 (a) and q-1 (b), 2-sum (c) and cells (x) of row q-1
struct Level {
  uint32_t a0, a1, b0, b1, c0, c1, x;
};

}  // namespace

template <int K, bool RES>
__global__ __launch_bounds__(256) void life_rule_bits(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                      Geo g, uint32_t birth, uint32_t survive, int zc, int XT,
                                                      int ntasks, double* __restrict__ resid) {
  constexpr int CW = 32;        // cells per lane
  constexpr int SEG = 62 * CW;  // owned cells per wave
  static_assert(K >= 1 && K <= CW, "generations must not reach past the halo lanes");
  const int lane = threadIdx.x & 63;
  const int task = (int)xcd_remap(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (task >= ntasks) return;  // wave-uniform, no barriers
  const int xt = task % XT, zt = task / XT;
  const int64_t x = (int64_t)xt * SEG - CW + (int64_t)lane * CW;
  const int64_t zs = g.lz_begin + (int64_t)zt * zc;
  const int64_t ze = min(g.lz_end, zs + (int64_t)zc);
  // pitch is a multiple of 256 cells, x of 32: a lane is wholly inside the row or wholly outside
  const bool xin = x >= 0 && x < g.pitch;
  const bool own = lane >= 1 && lane <= 62 && xin;
  const int64_t plane = g.plane;
  // held cells (x + j == 0 or x + j >= nx - 1) and cells inside the grid (x + j < nx)
  const int64_t hf = g.nx - 1 - x, vf = g.nx - x;
  const uint32_t hm = (x == 0 ? 1u : 0u) | (hf <= 0 ? ~0u : hf >= 32 ? 0u : ~0u << hf);
  const uint32_t vm = vf >= 32 ? ~0u : vf <= 0 ? 0u : (1u << vf) - 1u;
  // the rule's leaves, 0 / ~0 per table bit, with the held cells folded in: held = survives, never born
  uint32_t S[9], B[9];
#pragma unroll
  for (int n = 0; n < 9; ++n) {
    S[n] = (0u - ((survive >> n) & 1u)) | hm;
    B[n] = (0u - ((birth >> n) & 1u)) & ~hm;
  }
  // lanes outside the row read the nearest in-row vectors, rows past the storage its last row:
  // finite values that only meet halo lanes or held cells
  const uint8_t* ib = in + (x < 0 ? 0 : x >= g.pitch ? g.pitch - CW : x);
  auto ld = [&](int64_t lz) -> uint32_t {
    const int64_t lzc = lz < 0 ? 0 : lz >= g.lz_max ? g.lz_max - 1 : lz;
    dcheck(g, in, ib + lzc * plane, CW);
    const uint4* p = (const uint4*)(ib + lzc * plane);
    const uint4 a = p[0], b = p[1];
    return life_pack4(a.x) | life_pack4(a.y) << 4 | life_pack4(a.z) << 8 | life_pack4(a.w) << 12 |
           life_pack4(b.x) << 16 | life_pack4(b.y) << 20 | life_pack4(b.z) << 24 | life_pack4(b.w) << 28;
  };
  Level lv[K];  // level l = 1..K at index l - 1
#pragma unroll
  for (int l = 0; l < K; ++l) lv[l] = Level{0, 0, 0, 0, 0, 0, 0};
  // 2-sum and 3-sum of a row of cells; the cell beyond the lane through a DPP lane shift
  auto sums = [&](uint32_t X, uint32_t& s0, uint32_t& s1, uint32_t& c0, uint32_t& c1) {
    const uint32_t up = (uint32_t)lane_up1((int)X), dn = (uint32_t)lane_down1((int)X);
    const uint32_t L = __builtin_amdgcn_alignbit(X, up, 31);  // cell x + j - 1
    const uint32_t R = __builtin_amdgcn_alignbit(dn, X, 1);   // cell x + j + 1
    c0 = L ^ R;
    c1 = L & R;
    s0 = xor3(L, X, R);
    s1 = maj3(L, X, R);
  };
  {
    const uint32_t a = ld(zs - K - 1), b = ld(zs - K);
    uint32_t t0, t1;
    sums(a, lv[0].a0, lv[0].a1, t0, t1);
    sums(b, lv[0].b0, lv[0].b1, lv[0].c0, lv[0].c1);
    lv[0].x = b;
  }
  uint32_t nxt = ld(zs - K + 1);
  double acc = 0.0;
  for (int64_t q = zs - K + 1; q <= ze - 1 + K; ++q) {
    uint32_t X = nxt;  // generation 0 of row q
    nxt = ld(q + 1);
    const int64_t lz = q - K;
#pragma unroll
    for (int l = 1; l <= K; ++l) {
      Level& v = lv[l - 1];
      uint32_t s0, s1, c0, c1;
      sums(X, s0, s1, c0, c1);
      const uint32_t self = v.x;
      const int64_t gz = q - l + g.gz_off;  // the row this level finishes
      const bool bnd = l < K ? (gz <= 0 || gz >= g.gnz - 1) : (gz == 0 || gz == g.gnz - 1);
      uint32_t o = self;
      if (!bnd) {
        // N = (a0 + 2 a1) + (s0 + 2 s1) + (c0 + 2 c1), the neighbours of row q - l
        const uint32_t n0 = xor3(v.a0, s0, v.c0);
        const uint32_t k0 = maj3(v.a0, s0, v.c0);
        const uint32_t z1 = xor3(v.a1, s1, v.c1);
        const uint32_t k1a = maj3(v.a1, s1, v.c1);
        const uint32_t n1 = z1 ^ k0;
        const uint32_t k1b = z1 & k0;
        const uint32_t n2 = k1a ^ k1b;
        const uint32_t n3 = k1a & k1b;  // N == 8
        // next = self ? survive[N] : birth[N]
        const uint32_t m01 = bsel(n0, bsel(self, S[1], B[1]), bsel(self, S[0], B[0]));
        const uint32_t m23 = bsel(n0, bsel(self, S[3], B[3]), bsel(self, S[2], B[2]));
        const uint32_t m45 = bsel(n0, bsel(self, S[5], B[5]), bsel(self, S[4], B[4]));
        const uint32_t m67 = bsel(n0, bsel(self, S[7], B[7]), bsel(self, S[6], B[6]));
        const uint32_t m03 = bsel(n1, m23, m01);
        const uint32_t m47 = bsel(n1, m67, m45);
        o = bsel(n3, bsel(self, S[8], B[8]), bsel(n2, m47, m03));
      }
      v.a0 = v.b0;
      v.a1 = v.b1;
      v.b0 = s0;
      v.b1 = s1;
      v.c0 = c0;
      v.c1 = c1;
      v.x = X;
      if (l < K) {
        X = o;
      } else if (lz >= zs && own) {
        uint4 qa, qb;
        qa.x = life_unpack4(o, 0);
        qa.y = life_unpack4(o, 1);
        qa.z = life_unpack4(o, 2);
        qa.w = life_unpack4(o, 3);
        qb.x = life_unpack4(o, 4);
        qb.y = life_unpack4(o, 5);
        qb.z = life_unpack4(o, 6);
        qb.w = life_unpack4(o, 7);
        uint4* p = (uint4*)(out + lz * plane + x);
        dcheck(g, (const uint8_t*)out, (const uint8_t*)p, CW);
        p[0] = qa;
        p[1] = qb;
        if (RES) acc += (double)__builtin_popcount((o ^ self) & vm);
      }
    }
  }
  if (RES) wave_atomic_add(resid, acc);
}

template <int K>
static void launch_life_rule_k(const Geo& g, const uint8_t* in, uint8_t* out, uint32_t birth, uint32_t survive,
                               double* resid, hipStream_t s) {
  const int64_t planes = g.lz_end - g.lz_begin;
  if (planes <= 0) return;
  constexpr int SEG = 62 * 32;
  const int XT = (int)((g.nx + SEG - 1) / SEG);
  const int zc = pick_zc(planes, XT, 256, 4 * 2048);
  const int ZT = (int)((planes + zc - 1) / zc);
  const int ntasks = XT * ZT;
  const dim3 grd((unsigned)((ntasks + 3) / 4)), blk(256);
  if (resid)
    hipLaunchKernelGGL((life_rule_bits<K, true>), grd, blk, 0, s, in, out, g, birth, survive, zc, XT, ntasks, resid);
  else
    hipLaunchKernelGGL((life_rule_bits<K, false>), grd, blk, 0, s, in, out, g, birth, survive, zc, XT, ntasks, resid);
}

void launch_life_rule(const Geo& g, const uint8_t* in, uint8_t* out, uint32_t birth, uint32_t survive, int steps,
                      double* resid, hipStream_t s) {
  MDFX_CHECK(birth < 512u && survive < 512u, "a Life rule has 9 birth and 9 survival bits (0..8 neighbours)");
  switch (steps) {
    case 1: launch_life_rule_k<1>(g, in, out, birth, survive, resid, s); return;
    case 2: launch_life_rule_k<2>(g, in, out, birth, survive, resid, s); return;
    case 3: launch_life_rule_k<3>(g, in, out, birth, survive, resid, s); return;
    case 4: launch_life_rule_k<4>(g, in, out, birth, survive, resid, s); return;
    case 6: launch_life_rule_k<6>(g, in, out, birth, survive, resid, s); return;
    case 8: launch_life_rule_k<8>(g, in, out, birth, survive, resid, s); return;
    case 12: launch_life_rule_k<12>(g, in, out, birth, survive, resid, s); return;
    case 16: launch_life_rule_k<16>(g, in, out, birth, survive, resid, s); return;
    default: MDFX_FAIL(format("life: no %d-generation sweep for a rule table (1, 2, 3, 4, 6, 8, 12, 16)", steps));
  }
}

}  // namespace dev
}  // namespace mdfx
