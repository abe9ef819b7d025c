// 2D 9-point stencil with nine independent weights (conv9): u'(z, x) = sum of w[3*(dz+1) + (dx+1)] *
// u(z+dz, x+dx) over the 3x3 neighbourhood, one step (K = 1) or K fused steps (conv9_tbk) per sweep
// over memory. Any 3x3 linear update: upwind advection-diffusion, different conductivities in x and z,
// a full diffusion tensor (corner weights of opposite sign), blur, sharpening, decay.
//
// Arithmetic (sm::conv9_row / conv9_combine, shared with the CPU oracle and the naive kernel): an
// arriving row p with c = v(x), l = v(x-1), r = v(x+1) yields three horizontal sums, each one multiply
// and two fmas: T(p) = fma(w2, r, fma(w0, l, w1*c)) for output row p + 1, M(p) = fma(w5, r, fma(w3, l,
// w4*c)) for row p itself, B(p) = fma(w8, r, fma(w6, l, w7*c)) for row p - 1; u'(z) = (T(z-1) + M(z)) +
// B(z+1). Every arriving row computes its three sums ONCE and they feed three output rows: 9 multiplies
// or fmas and 2 adds per cell and level.
//
// How the rows are split (box9_tbk's division of work): each wave is an independent task, an x segment
// of 64 lanes x N cells (16 B per lane: N = 4 fp32 / 2 fp64) marching over zc rows; a block is four
// such tasks and has no barrier and no LDS. Segments OVERLAP by OV = ceil(K / N) lanes per side: a wave
// owns (and stores) only lanes OV .. 63 - OV. The x neighbours are DPP lane shifts, so the outermost
// column of a wave sees a 0 instead of its neighbour and every level corrupts one more column from
// outside; after K <= OV * N levels the owned lanes are still exact.
//
// What a level holds: level l = 1..K is a streaming recurrence over rows. Between two rows it keeps,
// for the newest complete row p of its input u_{l-1}: the pending sum P = T(p-1) + M(p) and T(p) itself
// (row p + 1 needs it); the last level also keeps the centre u_{K-1}(p) for the residual. When
// u_{l-1}(p+1) arrives, its l / c / r yield T(p+1), M(p+1), B(p+1); the level emits u_l(p) = P + B(p+1)
// into level l + 1 and rolls forward: P = T(p) + M(p+1), T = T(p+1). Two rows of registers per level.
//
// Weights and held cells (what differs from box9): the nine weights are WAVE-UNIFORM and stay in
// scalar registers (9 SGPRs fp32, 18 fp64; every multiply and fma reads one of them, which is what a
// gfx950 VALU op may read). box9's held-column trick, per-cell weights in VGPRs, would cost 9 x N = 36
// VGPRs here (box9: 12), which the K = 8 instances (two rows of state per level, 2 waves per SIMD at
// <= 256 VGPRs) do not have. Instead a held cell is a SELECT against the level's centre at the two
// places a row passes through P: a held cell (column x = 0 or x >= nx - 1, or a row at the global z
// boundary) keeps its centre in P in place of the pending sum and is emitted as it is. The column masks
// are loop-invariant lane masks in scalar register pairs, the row tests are wave-uniform and OR into
// them, so a held cell costs two v_cndmask per level and no VGPR, and comes out exactly as it went in
// for EVERY value (-0, and whatever its neighbours hold; a weight of 0 times a neighbour would not).
// Only tasks that touch a held cell pay for them: a task whose 64 lanes hold no edge column and whose
// whole pipeline is interior in z (all but the first and last segment of a row and the first and last
// chunk of a slab) runs a loop copy with neither test: 11 VALU ops per cell and level.
//
// Loads are not lane-predicated but clamped into the row / the storage, so every lane holds finite
// values. What is stored: level K's rows zs .. ze - 1 of the chunk, owned lanes only, non-temporal.
// The field is read once (+ the 2 * OV overlap lanes of 64 and K priming rows per chunk end) and
// written once per K steps.
//
// Region contract: output storage rows [lz_begin, lz_end) need u0 valid on [lz_begin - K, lz_end + K).
#include <algorithm>
#include <type_traits>

#include "kcommon.hpp"
#include "launchers.hpp"
#include "mdfx/kernels.hpp"
#include "mdfx/stencil_math.hpp"

namespace mdfx {
namespace dev {

// one lane's 16-B slice of a row
template <class T>
struct RowC9 {
  T v[VT<T>::N];
};

template <class T, int K, bool RES>
__global__ __launch_bounds__(256) void conv9_tbk(const T* __restrict__ in, T* __restrict__ out, Geo g,
                                                 sm::Conv9W<T> kw, int zc, int XT, int ntasks,
                                                 double* __restrict__ resid) {
  using V = typename VT<T>::type;
  using Row = RowC9<T>;
  constexpr int N = VT<T>::N;
  constexpr int OV = (K + N - 1) / N;     // overlap lanes per side
  constexpr int SEG = (64 - 2 * OV) * N;  // owned columns per wave
  constexpr int PD = 2;                   // u0 rows in flight (the row loop is unrolled by as many)
  const int lane = threadIdx.x & 63;
  // wave-uniform task index in an SGPR, so every row index and row test below is scalar
  const int task = (int)xcd_remap(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (task >= ntasks) return;  // wave-uniform; no block barriers in this kernel
  const int xt = task % XT, zt = task / XT;
  const int64_t x0 = (int64_t)xt * SEG - OV * N;  // the wave's first column (scalar)
  const int64_t x = x0 + (int64_t)lane * N;
  const int64_t zs = g.lz_begin + (int64_t)zt * zc;
  const int64_t ze = min(g.lz_end, zs + (int64_t)zc);
  const bool own = lane >= OV && lane <= 63 - OV && x >= 0 && x < g.pitch;
  const int64_t plane = g.plane;
  // held columns: loop-invariant lane masks
  bool held[N];
#pragma unroll
  for (int e = 0; e < N; ++e) held[e] = (x + e == 0) || (x + e >= g.nx - 1);
  // Loads without lane predication: lanes outside the row read the nearest in-row vector and rows
  // past the storage read its nearest row. Those values only ever meet held or unowned cells (the
  // left halo lanes of the first segment feed only x = 0, which is held; lanes beyond the row feed
  // only x >= nx - 1 and themselves).
  const T* ib = in + (x < 0 ? 0 : x >= g.pitch ? g.pitch - N : x);
  auto ld = [&](int64_t lz) -> Row {
    const int64_t lzc = lz < 0 ? 0 : lz >= g.lz_max ? g.lz_max - 1 : lz;
    dcheck(g, in, ib + lzc * plane, N);
    const V v = *(const V*)(ib + lzc * plane);  // one 16-B vector
    Row r;
#pragma unroll
    for (int e = 0; e < N; ++e) r.v[e] = v[e];
    return r;
  };
  Row P[K], TK[K];  // level l = 1..K at index l - 1: the pending sum and T of its newest row
  Row CK;           // the last level's centre u_{K-1}(p), for the residual
#pragma unroll
  for (int l = 0; l < K; ++l)
#pragma unroll
    for (int e = 0; e < N; ++e) P[l].v[e] = TK[l].v[e] = T(0);
#pragma unroll
  for (int e = 0; e < N; ++e) CK.v[e] = T(0);
  double acc = 0.0;
  const int64_t qlast = ze - 1 + K;
  // newest u0 row q; level l finishes row q - l (each level's first two rows are priming garbage
  // that no level needs). A task with no held cell at all (pipeline rows zs - K - 1 .. ze + K interior
  // in z, and no edge column among the wave's 64 * N) takes the loop copy without the hold selects.
  const bool zint = zs - K - 1 + g.gz_off >= 1 && ze + K + g.gz_off <= g.gnz - 2;
  const bool xint = x0 >= 1 && x0 + 64 * N <= g.nx - 1;
  Row nxr[PD];
#pragma unroll
  for (int i = 0; i < PD; ++i) nxr[i] = ld(zs - K + i);
  auto row_step = [&](int64_t q, auto hold, auto slot) __attribute__((always_inline)) {
    constexpr bool HT = decltype(hold)::value;
    constexpr int SL = decltype(slot)::value;  // which in-flight row is row q
    Row X = nxr[SL];
    nxr[SL] = ld(q + PD);
#pragma unroll
    for (int l = 1; l <= K; ++l) {
      const int64_t row = q - l;  // the row this level finishes
      const int64_t gz = row + g.gz_off;
      // wave-uniform: is the finished row p held, and the arriving row p + 1?
      const bool zh = HT && (gz <= 0 || gz >= g.gnz - 1);
      const bool zhn = HT && (gz + 1 <= 0 || gz + 1 >= g.gnz - 1);
      const T lft = lane_up1(X.v[N - 1]);
      const T rgt = lane_down1(X.v[0]);
      const Row c = CK;
      Row o;
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const T cl = e == 0 ? lft : X.v[e - 1], cr = e == N - 1 ? rgt : X.v[e + 1];
        const T tn = sm::conv9_row<T>(X.v[e], cl, cr, kw.w[0], kw.w[1], kw.w[2]);
        const T mn = sm::conv9_row<T>(X.v[e], cl, cr, kw.w[3], kw.w[4], kw.w[5]);
        const T bn = sm::conv9_row<T>(X.v[e], cl, cr, kw.w[6], kw.w[7], kw.w[8]);
        const T u = P[l - 1].v[e] + bn;  // sm::conv9_combine: (T(p-1) + M(p)) + B(p+1)
        const T pn = TK[l - 1].v[e] + mn;
        // a held cell keeps its centre in P instead of the pending sum, and is emitted as it is
        o.v[e] = (HT && (zh || held[e])) ? P[l - 1].v[e] : u;
        P[l - 1].v[e] = (HT && (zhn || held[e])) ? X.v[e] : pn;
        TK[l - 1].v[e] = tn;
      }
      if (RES && l == K) CK = X;
      if (l < K) {
        X = o;
      } else if (row >= zs && q <= qlast && own) {
        V ov;
#pragma unroll
        for (int e = 0; e < N; ++e) ov[e] = o.v[e];
        dcheck(g, (const T*)out, out + row * plane + x, N);
        store_nt((V*)(out + row * plane + x), ov);
        if (RES) {
#pragma unroll
          for (int e = 0; e < N; ++e)
            if (x + e < g.nx) {
              const double d = (double)o.v[e] - (double)c.v[e];
              acc += d * d;
            }
        }
      }
    }
  };
  auto march = [&](auto hold) __attribute__((always_inline)) {
    // an odd row count ends with one extra row (q = qlast + 1): loads clamp, nothing is stored
    for (int64_t q = zs - K; q <= qlast; q += 2) {
      row_step(q, hold, std::integral_constant<int, 0>{});
      row_step(q + 1, hold, std::integral_constant<int, 1>{});
    }
  };
  if (zint && xint)
    march(std::integral_constant<bool, false>{});
  else
    march(std::integral_constant<bool, true>{});
  if (RES) wave_atomic_add(resid, acc);
}

template <class T, int K>
static void launch_conv9_k(const Geo& g, const T* in, T* out, const StencilCoef& cf, double* resid, hipStream_t s) {
  const int64_t planes = g.lz_end - g.lz_begin;
  if (planes <= 0) return;
  constexpr int N = VT<T>::N, OV = (K + N - 1) / N, SEG = (64 - 2 * OV) * N;
  const int XT = (int)((g.nx + SEG - 1) / SEG);
  const int zc = pick_zc(planes, XT, 256, 4 * 2048);
  const int ZT = (int)((planes + zc - 1) / zc);
  const int ntasks = XT * ZT;
  const dim3 grd((unsigned)((ntasks + 3) / 4)), blk(256);
  sm::Conv9W<T> kw;
  for (int i = 0; i < 9; ++i) kw.w[i] = (T)cf.w9[i];
  if (resid)
    hipLaunchKernelGGL((conv9_tbk<T, K, true>), grd, blk, 0, s, in, out, g, kw, zc, XT, ntasks, resid);
  else
    hipLaunchKernelGGL((conv9_tbk<T, K, false>), grd, blk, 0, s, in, out, g, kw, zc, XT, ntasks, resid);
}

// steps = 1 or one of the 2D fused depths 2, 3, 4, 6, 8 (hip_supports_steps)
template <class T>
void launch_conv9(const Geo& g, const T* in, T* out, const StencilCoef& cf, int steps, double* resid, hipStream_t s) {
  switch (steps) {
    case 1: launch_conv9_k<T, 1>(g, in, out, cf, resid, s); break;
    case 2: launch_conv9_k<T, 2>(g, in, out, cf, resid, s); break;
    case 3: launch_conv9_k<T, 3>(g, in, out, cf, resid, s); break;
    case 4: launch_conv9_k<T, 4>(g, in, out, cf, resid, s); break;
    case 6: launch_conv9_k<T, 6>(g, in, out, cf, resid, s); break;
    case 8: launch_conv9_k<T, 8>(g, in, out, cf, resid, s); break;
    default: MDFX_FAIL(format("no conv9 kernel fuses %d steps (1, 2, 3, 4, 6, 8)", steps));
  }
}
template void launch_conv9<float>(const Geo&, const float*, float*, const StencilCoef&, int, double*, hipStream_t);
template void launch_conv9<double>(const Geo&, const double*, double*, const StencilCoef&, int, double*, hipStream_t);

}  // namespace dev
}  // namespace mdfx
