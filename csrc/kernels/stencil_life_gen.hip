// Generations rules (B/S/C: Brian's Brain B2/S/C3, Star Wars B2/S345/C4, ...), K generations per
// sweep, bit-sliced over P state planes: life_gen_bits.
//
// A cell holds a state s in 0 .. C-1: 0 dead, 1 alive, 2 .. C-1 dying. N counts the Moore neighbours
// whose state is exactly 1. Dead: 1 if birth[N] else 0. Alive: 1 if survive[N] else 2 % C. Dying:
// (s + 1) % C. C = 2 is a Life-like rule and never comes here (life_rule_bits, stencil_life.hip); this
// kernel serves C = 3 .. 32 at every built depth, single steps included. Cells >= C are the caller's
// error: they are treated as some state below 2^P and fault nothing.
//
// State encoding. P = ceil(log2 C) words per lane and row, plane b holding bit b of the state of 32
// cells (bit j = cell x + j). With s < C: the dying cells are D = p1 | .. | p(P-1), the alive plane is
// A = p0 & ~D, and only A is ever counted. The load takes plane b of 4 cells out of a u32 as
// (d & 0x01010101 << b) * 0x01020408 (life_pack4's multiply-gather with the shift left inside the
// product: v_and, v_mul_lo, v_bfe, v_lshl_or); the store scatters each nibble back with one multiply by
// 0x00204081 << b (v_bfe, v_mul_lo, v_and_or). 4 P and 3 P ops per 4 cells, once per sweep.
//
// Division of work: life_rule_bits', unchanged. One wave per task, no LDS, no barriers; 32 cells per
// lane, 62 owned lanes per segment (1,984 cells), one halo lane per side; the x neighbours of the alive
// plane through DPP lane shifts and v_alignbit; K levels of streaming row state in registers: the
// 3-sums of the alive planes of a level's last two input rows, the 2-sum, the alive plane and the P
// planes of the last one (7 + P words per level).
//
// One generation of 32 cells, on top of life_rule_bits' 32 ops (2 DPP + 2 v_alignbit + 4 row sums, 7
// for the exact 4-bit count, 17 selects with self = A):
//   m   = A ? survive[N] : birth[N]      the multiplexer tree, held cells folded into its leaves
//   r   = m & ~D                         the cells that are 1 next: birth is masked where dying
//   inc = D | (A & ~m)                   dying cells and failed survivors advance
//   W   = AND_b ~(p_b ^ E_b)             s == C-1, E_b = 0 / ~0 from bit b of C-1 (wave-uniform): P ops
//   G   = (inc & ~W) | hm                advancing and not wrapping to 0; or held
//   u   = p0 ^ hm, cy1 = u & ~hm         the increment's carry-in is 1 for an advancing cell and 0 for a
//   o_0 = (G & ~u) | r                   held one, whose planes then pass through G & (p_b ^ 0) = p_b:
//   o_b = G & (p_b ^ cy_b), cy_b+1 = cy_b & p_b      all P planes of a held cell are kept for 2 ops
//   D: P - 2 ops, o_b and the carries: 2 P - 3: 4 P + 3 boolean ops in all by the source. The gfx950
//   assembly (VALU instructions a further level adds to the kernel, K = 2 against K = 3, which also
//   counts the P + 1 selects that pass a held row through and the compiler's moves; a count of
//   instructions, not a measurement): 62 / 71 / 77 / 85 for P = 2 / 3 / 4 / 5 against 47 for
//   life_rule_bits by the same count, 1.32 / 1.51 / 1.64 / 1.81 of it. The alive plane of a level's
//   output is r itself (a held cell's r is its A), so only the loaded row pays for D and A.
//   Residual: popcount of OR_b (p_b ^ o_b) over the cells inside the grid, at the last level.
//
// Exactness. The neighbourhood radius is 1 and a cell's next state depends on its own state and the
// alive planes of its neighbours only, so life_rule_bits' overlap argument holds word for word with
// "word" read as "the P words of a lane": the halo lanes go wrong from the outside in by one cell per
// generation (K <= 32), rows need K valid ghost rows, and whatever a B0 rule or a dying cell does in
// padding stays there because pad cells, frame columns and rows, and rows outside the grid are HELD,
// with all their planes, by hm or by the wave-uniform row test.
//
// Resources (scripts/kernel_resources.py; VGPRs without / with the residual, K = 1, 2, 3, 4, 6, 8):
//   P = 2   54 / 60, 63 / 68, 74 / 77, 83 / 87, 105 / 109, 127 / 131      waves per SIMD 8, 8-7, 6, 5, 4, 4-3
//   P = 3   59 / 63, 69 / 73, 79 / 83, 91 / 94, 113 / 117, 137 / 141      8, 7-6, 6-5, 5, 4, 3
//   P = 4   64 / 66, 75 / 77, 86 / 88, 97 / 99, 121 / 125, 147 / 151      8-7, 6, 5, 4, 4, 3
//   P = 5   69 / 71, 81 / 83, 93 / 95, 105 / 107, 129 / 133, 157 / 161    7, 5, 5, 4, 3, 3
// No instance spills or uses scratch or LDS. K = 12 / 16 are not built: K = 8 is already bound by the
// arithmetic at every P (below), and K = 12 would need about 170 VGPRs at P = 2, under 3 waves per SIMD.
//
// Measured on one MI355X, 32768^2, density 0.5, against life_rule_bits (HighLife) at equal K, alternating
// in one process, best of 5 rounds of 100 sweeps, spread within 0.5 %, two runs within 0.5 % of each other
// (GCells/s; profiles/r12_life_generations/). Every kernel moves one byte in and one out per cell per sweep:
//     K                    1      2      3      4       6       8
//     life_rule_bits    2254   4461   6596   8679   12721   16262
//     C = 3  (P = 2)    2160   4238   6415   8577   12288   14581     0.96 0.95 0.97 0.99 0.97 0.90
//     C = 8  (P = 3)    2138   4213   6407   8478   11260   11794     0.95 0.94 0.97 0.98 0.89 0.73
//     C = 16 (P = 4)    2106   4288   6349   8022    9707   10257     0.93 0.96 0.96 0.92 0.76 0.63
//     C = 32 (P = 5)    2089   4212   5890   6948    8208    8983     0.93 0.94 0.89 0.80 0.65 0.55
// A sweep costs one pass over memory up to K = 6 / 4 / 4 / 2 for P = 2 / 3 / 4 / 5 and is bound by the
// arithmetic beyond; the deepest sweep is still the fastest per generation at every P, so the default
// depth is 8. The naive kernel runs C = 3 at 394 GCells/s, so single steps run here too.
#include <algorithm>
#include <type_traits>

#include "kcommon.hpp"
#include "launchers.hpp"
#include "mdfx/kernels.hpp"

namespace mdfx {
namespace dev {

namespace {

__device__ __forceinline__ uint32_t gsel(uint32_t c, uint32_t a, uint32_t b) { return (c & a) | (~c & b); }
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
__device__ __forceinline__ uint32_t gxor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ uint32_t gmaj3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
}
#else
__device__ __forceinline__ uint32_t gxor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
__device__ __forceinline__ uint32_t gmaj3(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }
#endif

// plane B of the four cells of a u32 -> bits 0..3
template <int B>
__device__ __forceinline__ uint32_t gen_pack4(uint32_t d) {
  return __builtin_amdgcn_ubfe((d & (0x01010101u << B)) * 0x01020408u, 24 + B, 4);
}

// per-level streaming state: 3-sums of the alive planes of rows q-2 (a) and q-1 (b), 2-sum (c), alive
// plane (A) and state planes (p) of row q-1
template <int P>
struct GenLevel {
  uint32_t a0, a1, b0, b1, c0, c1, A;
  uint32_t p[P];
};

}  // namespace

template <int K, int P, bool RES>
__global__ __launch_bounds__(256) void life_gen_bits(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                     Geo g, uint32_t birth, uint32_t survive, uint32_t last, int zc,
                                                     int XT, int ntasks, double* __restrict__ resid) {
  constexpr int CW = 32;        // cells per lane
  constexpr int SEG = 62 * CW;  // owned cells per wave
  static_assert(K >= 1 && K <= CW, "generations must not reach past the halo lanes");
  static_assert(P >= 2 && P <= 5, "2 .. 5 state planes (3 .. 32 states)");
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
  // the rule's leaves, 0 / ~0 per table bit, with the held cells folded in: a held cell's m is its A
  uint32_t S[9], B[9];
#pragma unroll
  for (int n = 0; n < 9; ++n) {
    S[n] = (0u - ((survive >> n) & 1u)) | hm;
    B[n] = (0u - ((birth >> n) & 1u)) & ~hm;
  }
  // bit b of C - 1, 0 / ~0 (wave-uniform)
  uint32_t E[P];
#pragma unroll
  for (int b = 0; b < P; ++b) E[b] = 0u - ((last >> b) & 1u);
  // lanes outside the row read the nearest in-row vectors, rows past the storage its last row:
  // finite values that only meet halo lanes or held cells
  const uint8_t* ib = in + (x < 0 ? 0 : x >= g.pitch ? g.pitch - CW : x);
  auto ld = [&](int64_t lz, uint32_t* p) {
    const int64_t lzc = lz < 0 ? 0 : lz >= g.lz_max ? g.lz_max - 1 : lz;
    dcheck(g, in, ib + lzc * plane, CW);
    const uint4* v = (const uint4*)(ib + lzc * plane);
    const uint4 a = v[0], b = v[1];
    auto pk = [&](auto bc) {
      constexpr int Bb = decltype(bc)::value;
      p[Bb] = gen_pack4<Bb>(a.x) | gen_pack4<Bb>(a.y) << 4 | gen_pack4<Bb>(a.z) << 8 | gen_pack4<Bb>(a.w) << 12 |
              gen_pack4<Bb>(b.x) << 16 | gen_pack4<Bb>(b.y) << 20 | gen_pack4<Bb>(b.z) << 24 |
              gen_pack4<Bb>(b.w) << 28;
    };
    pk(std::integral_constant<int, 0>{});
    pk(std::integral_constant<int, 1>{});
    if constexpr (P > 2) pk(std::integral_constant<int, 2>{});
    if constexpr (P > 3) pk(std::integral_constant<int, 3>{});
    if constexpr (P > 4) pk(std::integral_constant<int, 4>{});
  };
  // the dying cells and the alive plane of a row of states
  auto dying = [&](const uint32_t* p) -> uint32_t {
    uint32_t d = p[1];
#pragma unroll
    for (int b = 2; b < P; ++b) d |= p[b];
    return d;
  };
  GenLevel<P> lv[K];  // level l = 1..K at index l - 1
#pragma unroll
  for (int l = 0; l < K; ++l) {
    lv[l].a0 = lv[l].a1 = lv[l].b0 = lv[l].b1 = lv[l].c0 = lv[l].c1 = lv[l].A = 0;
#pragma unroll
    for (int b = 0; b < P; ++b) lv[l].p[b] = 0;
  }
  // 2-sum and 3-sum of a row's alive plane; the cell beyond the lane through a DPP lane shift
  auto sums = [&](uint32_t X, uint32_t& s0, uint32_t& s1, uint32_t& c0, uint32_t& c1) {
    const uint32_t up = (uint32_t)lane_up1((int)X), dn = (uint32_t)lane_down1((int)X);
    const uint32_t L = __builtin_amdgcn_alignbit(X, up, 31);  // cell x + j - 1
    const uint32_t R = __builtin_amdgcn_alignbit(dn, X, 1);   // cell x + j + 1
    c0 = L ^ R;
    c1 = L & R;
    s0 = gxor3(L, X, R);
    s1 = gmaj3(L, X, R);
  };
  {
    uint32_t a[P], b[P];
    ld(zs - K - 1, a);
    ld(zs - K, b);
    const uint32_t aA = a[0] & ~dying(a), bA = b[0] & ~dying(b);
    uint32_t t0, t1;
    sums(aA, lv[0].a0, lv[0].a1, t0, t1);
    sums(bA, lv[0].b0, lv[0].b1, lv[0].c0, lv[0].c1);
    lv[0].A = bA;
#pragma unroll
    for (int i = 0; i < P; ++i) lv[0].p[i] = b[i];
  }
  uint32_t nxt[P];
  ld(zs - K + 1, nxt);
  double acc = 0.0;
  for (int64_t q = zs - K + 1; q <= ze - 1 + K; ++q) {
    uint32_t X[P];  // generation 0 of row q
#pragma unroll
    for (int i = 0; i < P; ++i) X[i] = nxt[i];
    ld(q + 1, nxt);
    uint32_t XA = X[0] & ~dying(X);
    const int64_t lz = q - K;
#pragma unroll
    for (int l = 1; l <= K; ++l) {
      GenLevel<P>& v = lv[l - 1];
      uint32_t s0, s1, c0, c1;
      sums(XA, s0, s1, c0, c1);
      const uint32_t self = v.A;
      const int64_t gz = q - l + g.gz_off;  // the row this level finishes
      const bool bnd = l < K ? (gz <= 0 || gz >= g.gnz - 1) : (gz == 0 || gz == g.gnz - 1);
      uint32_t o[P], oA = self;
#pragma unroll
      for (int i = 0; i < P; ++i) o[i] = v.p[i];
      if (!bnd) {
        // N = (a0 + 2 a1) + (s0 + 2 s1) + (c0 + 2 c1), the alive neighbours of row q - l
        const uint32_t n0 = gxor3(v.a0, s0, v.c0);
        const uint32_t k0 = gmaj3(v.a0, s0, v.c0);
        const uint32_t z1 = gxor3(v.a1, s1, v.c1);
        const uint32_t k1a = gmaj3(v.a1, s1, v.c1);
        const uint32_t n1 = z1 ^ k0;
        const uint32_t k1b = z1 & k0;
        const uint32_t n2 = k1a ^ k1b;
        const uint32_t n3 = k1a & k1b;  // N == 8
        // m = alive ? survive[N] : birth[N]
        const uint32_t m01 = gsel(n0, gsel(self, S[1], B[1]), gsel(self, S[0], B[0]));
        const uint32_t m23 = gsel(n0, gsel(self, S[3], B[3]), gsel(self, S[2], B[2]));
        const uint32_t m45 = gsel(n0, gsel(self, S[5], B[5]), gsel(self, S[4], B[4]));
        const uint32_t m67 = gsel(n0, gsel(self, S[7], B[7]), gsel(self, S[6], B[6]));
        const uint32_t m03 = gsel(n1, m23, m01);
        const uint32_t m47 = gsel(n1, m67, m45);
        const uint32_t m = gsel(n3, gsel(self, S[8], B[8]), gsel(n2, m47, m03));
        const uint32_t D = dying(v.p);
        const uint32_t r = m & ~D;             // 1 next: born, or survived
        const uint32_t inc = D | (self & ~m);  // advances: dying, or failed to survive
        uint32_t W = ~(v.p[0] ^ E[0]);         // s == C - 1: wraps to 0
#pragma unroll
        for (int b = 1; b < P; ++b) W &= ~(v.p[b] ^ E[b]);
        const uint32_t G = (inc & ~W) | hm;
        const uint32_t u = v.p[0] ^ hm;  // a held cell: ~p0, carry 0, so every plane passes through
        uint32_t cy = u & ~hm;
        o[0] = (G & ~u) | r;
#pragma unroll
        for (int b = 1; b < P; ++b) {
          o[b] = G & (v.p[b] ^ cy);
          cy &= v.p[b];
        }
        oA = r;
      }
      v.a0 = v.b0;
      v.a1 = v.b1;
      v.b0 = s0;
      v.b1 = s1;
      v.c0 = c0;
      v.c1 = c1;
      if (l == K && RES && lz >= zs && own) {
        uint32_t ch = o[0] ^ v.p[0];
#pragma unroll
        for (int b = 1; b < P; ++b) ch |= o[b] ^ v.p[b];
        acc += (double)__builtin_popcount(ch & vm);
      }
      v.A = XA;
#pragma unroll
      for (int i = 0; i < P; ++i) v.p[i] = X[i];
      if (l < K) {
        XA = oA;
#pragma unroll
        for (int i = 0; i < P; ++i) X[i] = o[i];
      } else if (lz >= zs && own) {
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          w[k] = (__builtin_amdgcn_ubfe(o[0], 4 * k, 4) * 0x00204081u) & 0x01010101u;
#pragma unroll
          for (int b = 1; b < P; ++b)
            w[k] |= (__builtin_amdgcn_ubfe(o[b], 4 * k, 4) * (0x00204081u << b)) & (0x01010101u << b);
        }
        uint4* p = (uint4*)(out + lz * plane + x);
        dcheck(g, (const uint8_t*)out, (const uint8_t*)p, CW);
        p[0] = make_uint4(w[0], w[1], w[2], w[3]);
        p[1] = make_uint4(w[4], w[5], w[6], w[7]);
      }
    }
  }
  if (RES) wave_atomic_add(resid, acc);
}

template <int K, int P>
static void launch_life_gen_kp(const Geo& g, const uint8_t* in, uint8_t* out, uint32_t birth, uint32_t survive,
                               int states, double* resid, hipStream_t s) {
  const int64_t planes = g.lz_end - g.lz_begin;
  if (planes <= 0) return;
  constexpr int SEG = 62 * 32;
  const int XT = (int)((g.nx + SEG - 1) / SEG);
  const int zc = pick_zc(planes, XT, 256, 4 * 2048);
  const int ZT = (int)((planes + zc - 1) / zc);
  const int ntasks = XT * ZT;
  const dim3 grd((unsigned)((ntasks + 3) / 4)), blk(256);
  const uint32_t last = (uint32_t)states - 1u;
  if (resid)
    hipLaunchKernelGGL((life_gen_bits<K, P, true>), grd, blk, 0, s, in, out, g, birth, survive, last, zc, XT, ntasks,
                       resid);
  else
    hipLaunchKernelGGL((life_gen_bits<K, P, false>), grd, blk, 0, s, in, out, g, birth, survive, last, zc, XT, ntasks,
                       resid);
}

template <int P>
static void launch_life_gen_p(const Geo& g, const uint8_t* in, uint8_t* out, uint32_t birth, uint32_t survive,
                              int states, int steps, double* resid, hipStream_t s) {
  switch (steps) {
    case 1: launch_life_gen_kp<1, P>(g, in, out, birth, survive, states, resid, s); return;
    case 2: launch_life_gen_kp<2, P>(g, in, out, birth, survive, states, resid, s); return;
    case 3: launch_life_gen_kp<3, P>(g, in, out, birth, survive, states, resid, s); return;
    case 4: launch_life_gen_kp<4, P>(g, in, out, birth, survive, states, resid, s); return;
    case 6: launch_life_gen_kp<6, P>(g, in, out, birth, survive, states, resid, s); return;
    case 8: launch_life_gen_kp<8, P>(g, in, out, birth, survive, states, resid, s); return;
    default: MDFX_FAIL(format("life: no %d-generation sweep for a Generations rule (1, 2, 3, 4, 6, 8)", steps));
  }
}

bool life_gen_supported(int states, int steps) {
  return states >= 3 && states <= 32 && (steps == 1 || steps == 2 || steps == 3 || steps == 4 || steps == 6 || steps == 8);
}

void launch_life_gen(const Geo& g, const uint8_t* in, uint8_t* out, uint32_t birth, uint32_t survive, int states,
                     int steps, double* resid, hipStream_t s) {
  MDFX_CHECK(birth < 512u && survive < 512u, "a Life rule has 9 birth and 9 survival bits (0..8 neighbours)");
  MDFX_CHECK(states >= 3 && states <= 32, format("life_gen_bits serves 3 .. 32 states (got %d)", states));
  if (states <= 4)
    launch_life_gen_p<2>(g, in, out, birth, survive, states, steps, resid, s);
  else if (states <= 8)
    launch_life_gen_p<3>(g, in, out, birth, survive, states, steps, resid, s);
  else if (states <= 16)
    launch_life_gen_p<4>(g, in, out, birth, survive, states, steps, resid, s);
  else
    launch_life_gen_p<5>(g, in, out, birth, survive, states, steps, resid, s);
}

}  // namespace dev
}  // namespace mdfx
