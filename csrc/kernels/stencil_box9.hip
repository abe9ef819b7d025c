// 2D 9-point weighted stencil (box9): u' = c0*u + c1*(4 edge neighbours) + c2*(4 corner neighbours),
// one step (box9_wave = the K = 1 instance) or K fused steps (box9_tbk) per sweep over memory.
//
// Arithmetic (sm::box9_A / box9_B / box9_combine, shared with the CPU oracle and the naive kernel):
// a row contributes to the rows above and below through A = fma(c2, h, c1 * c) and to itself
// through B = fma(c1, h, c0 * c), h = v(x-1) + v(x+1); u'(z) = (A(z-1) + B(z)) + A(z+1). So every
// arriving row computes h, A and B ONCE and they feed three output rows.
//
// How the rows are split: each wave is an independent task, an x segment of 64 lanes x N cells
// (16 B per lane: N = 4 fp32 / 2 fp64) marching over zc rows; a block is four such tasks and has no
// barrier and no LDS. Segments OVERLAP by OV = ceil(K / N) lanes per side: a wave owns (and stores)
// only lanes OV .. 63 - OV, the outer lanes carry the neighbour segments' columns through the same
// instructions. The x neighbours are DPP lane shifts, so the outermost column of a wave sees a 0
// instead of its neighbour and every level corrupts one more column from outside; after
// K <= OV * N levels the owned lanes are still exact.
//
// What a level holds: level l = 1..K is a streaming recurrence over rows. Between two rows it
// keeps, for the newest complete row p of its input u_{l-1}: the pending sum P = A(p-1) + B(p) and
// A(p) itself (row p + 1 needs it); the last level also keeps the centre u_{K-1}(p) for the residual.
// When u_{l-1}(p+1) arrives, one h yields A(p+1) and B(p+1); the level emits u_l(p) = P + A(p+1) into
// level l + 1 and rolls forward: P = A(p) + B(p+1), A = A(p+1). Two rows of registers per level, no
// register rotation; the loop is unrolled by two rows and two u0 rows are in flight while one is
// consumed (a row of level work is far shorter than a global-load round trip).
//
// Held cells: the columns x = 0 and x >= nx - 1 carry per-cell coefficients (c0, c1, c2) = (1, 0, 0),
// so A = 0 and B = c there and u' = (0 + c) + 0 = c with no select (finite data; loads are not
// lane-predicated but clamped into the row / the storage, so every lane holds finite values). A row
// at the global z boundary keeps its centre in P in place of the pending sum and is emitted as it is
// (two wave-uniform selects per cell, exact for every value); chunks whose whole pipeline is interior
// in z run a loop copy without those tests.
//
// What is stored: level K's rows zs .. ze - 1 of the chunk, owned lanes only, non-temporal. The field
// is read once (+ the 2 * OV overlap lanes of 64 and K priming rows per chunk end) and written once
// per K steps.
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
struct Row9 {
  T v[VT<T>::N];
};

template <class T, int K, bool RES>
__global__ __launch_bounds__(256) void box9_tbk(const T* __restrict__ in, T* __restrict__ out, Geo g, T c0, T c1,
                                                T c2, int zc, int XT, int ntasks, double* __restrict__ resid) {
  using V = typename VT<T>::type;
  using Row = Row9<T>;
  constexpr int N = VT<T>::N;
  constexpr int OV = (K + N - 1) / N;     // overlap lanes per side
  constexpr int SEG = (64 - 2 * OV) * N;  // owned columns per wave
  constexpr int PD = 2;                   // u0 rows in flight (the row loop is unrolled by as many)
  const int lane = threadIdx.x & 63;
  // wave-uniform task index in an SGPR, so every row index and row test below is scalar
  const int task = (int)xcd_remap(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (task >= ntasks) return;  // wave-uniform; no block barriers in this kernel
  const int xt = task % XT, zt = task / XT;
  const int64_t x = (int64_t)xt * SEG - OV * N + (int64_t)lane * N;
  const int64_t zs = g.lz_begin + (int64_t)zt * zc;
  const int64_t ze = min(g.lz_end, zs + (int64_t)zc);
  const bool own = lane >= OV && lane <= 63 - OV && x >= 0 && x < g.pitch;
  const int64_t plane = g.plane;
  // per-cell coefficients: (1, 0, 0) on the held columns
  T k0[N], k1[N], k2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const bool held = (x + e == 0) || (x + e >= g.nx - 1);
    k0[e] = held ? T(1) : c0;
    k1[e] = held ? T(0) : c1;
    k2[e] = held ? T(0) : c2;
  }
  // Loads without lane predication: lanes outside the row read the nearest in-row vector and rows
  // past the storage read its nearest row. Those values are finite and only ever meet held or
  // unowned cells (the left halo lanes of the first segment feed only x = 0, which is held; lanes
  // beyond the row feed only x >= nx - 1 and themselves).
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
  Row P[K], A[K];  // level l = 1..K at index l - 1
  Row CK;          // the last level's centre u_{K-1}(p), for the residual
#pragma unroll
  for (int l = 0; l < K; ++l)
#pragma unroll
    for (int e = 0; e < N; ++e) P[l].v[e] = A[l].v[e] = T(0);
#pragma unroll
  for (int e = 0; e < N; ++e) CK.v[e] = T(0);
  double acc = 0.0;
  const int64_t qlast = ze - 1 + K;
  // newest u0 row q; level l finishes row q - l (each level's first two rows are priming garbage
  // that no level needs). Chunks whose pipeline rows zs - K - 1 .. ze + K are all interior in z take
  // the loop copy without the per-level row test.
  const bool zint = zs - K - 1 + g.gz_off >= 1 && ze + K + g.gz_off <= g.gnz - 2;
  Row nxr[PD];
#pragma unroll
  for (int i = 0; i < PD; ++i) nxr[i] = ld(zs - K + i);
  auto row_step = [&](int64_t q, auto ztest, auto slot) __attribute__((always_inline)) {
    constexpr bool ZT = decltype(ztest)::value;
    constexpr int SL = decltype(slot)::value;  // which in-flight row is row q
    Row X = nxr[SL];
    nxr[SL] = ld(q + PD);
#pragma unroll
    for (int l = 1; l <= K; ++l) {
      const int64_t row = q - l;  // the row this level finishes
      const int64_t gz = row + g.gz_off;
      // wave-uniform: is the finished row p held, and the arriving row p + 1? A held row keeps its
      // centre in P instead of the pending sum, and is emitted as it is
      const bool zh = ZT && (gz <= 0 || gz >= g.gnz - 1);
      const bool zhn = ZT && (gz + 1 <= 0 || gz + 1 >= g.gnz - 1);
      const T lft = lane_up1(X.v[N - 1]);
      const T rgt = lane_down1(X.v[0]);
      const Row c = CK;
      Row o;
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const T h = (e == 0 ? lft : X.v[e - 1]) + (e == N - 1 ? rgt : X.v[e + 1]);
        const T an = sm::box9_A<T>(X.v[e], h, k1[e], k2[e]);
        const T bn = sm::box9_B<T>(X.v[e], h, k0[e], k1[e]);
        const T u = P[l - 1].v[e] + an;  // sm::box9_combine: (A(p-1) + B(p)) + A(p+1)
        o.v[e] = zh ? P[l - 1].v[e] : u;
        P[l - 1].v[e] = zhn ? X.v[e] : A[l - 1].v[e] + bn;
        A[l - 1].v[e] = an;
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
  auto march = [&](auto ztest) __attribute__((always_inline)) {
    // an odd row count ends with one extra row (q = qlast + 1): loads clamp, nothing is stored
    for (int64_t q = zs - K; q <= qlast; q += 2) {
      row_step(q, ztest, std::integral_constant<int, 0>{});
      row_step(q + 1, ztest, std::integral_constant<int, 1>{});
    }
  };
  if (zint)
    march(std::integral_constant<bool, false>{});
  else
    march(std::integral_constant<bool, true>{});
  if (RES) wave_atomic_add(resid, acc);
}

template <class T, int K>
static void launch_box9_k(const Geo& g, const T* in, T* out, const StencilCoef& cf, double* resid, hipStream_t s) {
  const int64_t planes = g.lz_end - g.lz_begin;
  if (planes <= 0) return;
  constexpr int N = VT<T>::N, OV = (K + N - 1) / N, SEG = (64 - 2 * OV) * N;
  const int XT = (int)((g.nx + SEG - 1) / SEG);
  const int zc = pick_zc(planes, XT, 256, 4 * 2048);
  const int ZT = (int)((planes + zc - 1) / zc);
  const int ntasks = XT * ZT;
  const dim3 grd((unsigned)((ntasks + 3) / 4)), blk(256);
  const T c0 = (T)cf.c0, c1 = (T)cf.c1, c2 = (T)cf.c2;
  if (resid)
    hipLaunchKernelGGL((box9_tbk<T, K, true>), grd, blk, 0, s, in, out, g, c0, c1, c2, zc, XT, ntasks, resid);
  else
    hipLaunchKernelGGL((box9_tbk<T, K, false>), grd, blk, 0, s, in, out, g, c0, c1, c2, zc, XT, ntasks, resid);
}

// One cell per lane: the "naive" variant, the on-device oracle of the kernels above (dispatched by
// naive_launch, stencil_naive.hip). It is compiled here so that it shares this file's build flags.
template <class T, bool RES>
__global__ __launch_bounds__(256) void naive_box9(const T* __restrict__ in, T* __restrict__ out, Geo g, T c0, T c1,
                                                  T c2, double* __restrict__ resid) {
  const int64_t n = g.nx * (g.lz_end - g.lz_begin);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t x = i % g.nx, lz = g.lz_begin + i / g.nx;
    const int64_t gz = lz + g.gz_off;
    const int64_t idx = lz * g.plane + x;
    const T c = in[idx];
    T o = c;
    if (x > 0 && x < g.nx - 1 && gz > 0 && gz < g.gnz - 1) {
      const T *zm = in + idx - g.plane, *zp = in + idx + g.plane;
      const T am = sm::box9_A<T>(zm[0], zm[-1] + zm[1], c1, c2);
      const T bc = sm::box9_B<T>(c, in[idx - 1] + in[idx + 1], c0, c1);
      const T ap = sm::box9_A<T>(zp[0], zp[-1] + zp[1], c1, c2);
      o = sm::box9_combine<T>(am, bc, ap);
    }
    out[idx] = o;
    if (RES) {
      const double d = (double)o - (double)c;
      acc += d * d;
    }
  }
  if (RES) wave_atomic_add(resid, acc);
}

template <class T>
void launch_box9_naive(const Geo& g, const T* in, T* out, const StencilCoef& cf, double* resid, hipStream_t s) {
  const int64_t n = g.nx * (g.lz_end - g.lz_begin);
  if (n <= 0) return;
  const dim3 grd((unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32)), blk(256);
  const T c0 = (T)cf.c0, c1 = (T)cf.c1, c2 = (T)cf.c2;
  if (resid)
    hipLaunchKernelGGL((naive_box9<T, true>), grd, blk, 0, s, in, out, g, c0, c1, c2, resid);
  else
    hipLaunchKernelGGL((naive_box9<T, false>), grd, blk, 0, s, in, out, g, c0, c1, c2, resid);
}
template void launch_box9_naive<float>(const Geo&, const float*, float*, const StencilCoef&, double*, hipStream_t);
template void launch_box9_naive<double>(const Geo&, const double*, double*, const StencilCoef&, double*, hipStream_t);

// steps = 1 (box9_wave) or one of the 2D fused depths 2, 3, 4, 6, 8 (hip_supports_steps)
template <class T>
void launch_box9(const Geo& g, const T* in, T* out, const StencilCoef& cf, int steps, double* resid, hipStream_t s) {
  switch (steps) {
    case 1: launch_box9_k<T, 1>(g, in, out, cf, resid, s); break;
    case 2: launch_box9_k<T, 2>(g, in, out, cf, resid, s); break;
    case 3: launch_box9_k<T, 3>(g, in, out, cf, resid, s); break;
    case 4: launch_box9_k<T, 4>(g, in, out, cf, resid, s); break;
    case 6: launch_box9_k<T, 6>(g, in, out, cf, resid, s); break;
    case 8: launch_box9_k<T, 8>(g, in, out, cf, resid, s); break;
    default: MDFX_FAIL(format("no box9 kernel fuses %d steps (1, 2, 3, 4, 6, 8)", steps));
  }
}
template void launch_box9<float>(const Geo&, const float*, float*, const StencilCoef&, int, double*, hipStream_t);
template void launch_box9<double>(const Geo&, const double*, double*, const StencilCoef&, int, double*, hipStream_t);

}  // namespace dev
}  // namespace mdfx
