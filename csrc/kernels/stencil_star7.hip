// 3D 7-point star with seven independent weights (star7):
//   u' = c0*u + wxm*u(x-1) + wxp*u(x+1) + wym*u(y-1) + wyp*u(y+1) + wzm*u(z-1) + wzp*u(z+1),
// one step (the K = 1 instance) or K = 2, 3, 4 fused steps per sweep over memory (star7_tbk).
//
// Arithmetic (sm::star7_B / star7_P / star7_finish, shared with the CPU oracle and the naive kernel):
// one multiply and six fmas, ordered for the z march. B is the cell's own plane, P = fma(wzm, zm, B)
// is final the moment plane z has arrived, and one fma finishes u' = fma(wzp, zp, P) a plane later.
// There are no adds, so nothing can be contracted differently on host and device.
//
// How the work is split: every wave is an independent task; no LDS, no block barrier (a block is
// four tasks). A task is
//   - an x segment of 64 lanes x N cells (16 B per lane at K = 1, 8 B per lane for the fused depths,
//     so N = 4 / 2 fp32 and 2 / 1 fp64) with OV = ceil(K / N) overlap lanes per side: a wave owns (and
//     stores) only lanes OV .. 63 - OV. The x neighbours are DPP lane shifts, so the outermost column
//     of a wave sees a 0 instead of its neighbour and every level corrupts one more column from
//     outside; after K <= OV * N levels the owned lanes are still exact;
//   - a y strip of RY output rows, handled as a trapezoid inside the wave: u0 arrives in RY + 2K rows
//     and level l computes the RY + 2(K - l) rows y0 - (K - l) .. y0 + RY + (K - l) - 1 from the
//     RY + 2(K - l + 1) rows of level l - 1 (redundant rows instead of a seam exchange);
//   - a chunk of zc planes to march over (+ K priming planes at each end).
//
// What a level holds: per level and row, for the newest complete plane p of its input u_{l-1}, the
// pending P(p) and that plane's centre C = u_{l-1}(p), which is the zm of plane p + 1 (and, at the
// last level, the centre the residual needs). When plane q of u0 arrives, its rows cascade one by
// one through all K levels: row r of level l - 1 completes the 3-row window of row r - 2 of level l,
// which forms B and P(p + 1) from the window, finishes u_l(p) = fma(wzp, centre, P(p)), hands it to
// level l + 1 and rolls P and C forward. Everything is unrolled, so the windows are register names.
// The plane loop is unrolled by two and holds two u0 planes of registers: a row of plane q + 2 is
// requested as soon as the same row of plane q has fed its last level-1 row.
//
// Held cells: the columns x = 0 and x >= nx - 1 carry per-cell weights (c0, w...) = (1, 0, ..., 0), so
// B = P = u' = c with no select (finite data; loads are not lane-predicated but clamped into the row,
// the plane and the storage, so every lane holds finite values and a zero weight never meets an
// inf). A held row (y = 0, y >= ny - 1) or plane (global z boundary) is wave-uniform: its cells are
// emitted as the centre C itself, one select per cell, exact for every value. Chunks whose whole
// pipeline is interior in y and z run a loop copy without those tests.
//
// What is stored: level K's rows of the planes zs .. ze - 1 of the chunk, owned lanes only,
// non-temporal.
//
// Region contract: output storage planes [lz_begin, lz_end) need u0 valid on [lz_begin - K, lz_end + K).
// Slab geometry only (pencil layouts take single steps through naive_star7).
#include <algorithm>
#include <type_traits>

#include "kcommon.hpp"
#include "launchers.hpp"
#include "mdfx/kernels.hpp"
#include "mdfx/stencil_math.hpp"
#include "rowops.hpp"

namespace mdfx {
namespace dev {

// one lane's vector of a row: N elements in one 8- or 16-B access
template <class T, int N>
struct Vec7 {
  typedef T type __attribute__((ext_vector_type(N)));
  static __device__ __forceinline__ T get(const type& v, int e) { return v[e]; }
  static __device__ __forceinline__ void set(type& v, int e, T x) { v[e] = x; }
};
template <class T>
struct Vec7<T, 1> {
  typedef T type;
  static __device__ __forceinline__ T get(const type& v, int) { return v; }
  static __device__ __forceinline__ void set(type& v, int, T x) { v = x; }
};
template <class T, int N>
struct Row7 {
  T v[N];
};

// Tile constants per (T, K). Bytes per lane: 16 for the single step (it is bound by memory; the widest
// access), 8 for the fused depths (half the registers per row, so a wave holds the rows of K levels).
// RY: the strip's output rows. A level row costs 2 values (P, C) x N x sizeof(T) / 4 registers and the
// two u0 planes 2 x (RY + 2K) rows, and the allocator needs about twice that sum (the loop-carried rows
// rotate through registers), so the strips are short: deeper ones spilled. VGPRs: fp32 212 / 182 / 226 /
// 242 for K = 1 / 2 / 3 / 4, fp64 213 / 202 / 230 / 284. Row-update redundancy (K RY + K (K - 1)) / (K RY):
// 1.25 for K = 2, 1.67 (fp64 2.0) for K = 3, 4.0 for K = 4.
template <class T, int K>
struct Star7Tile {
  static constexpr int N = (K == 1 ? 16 : 8) / (int)sizeof(T);
  static constexpr int RY = K <= 2 ? 4 : K == 3 ? (sizeof(T) == 4 ? 3 : 2) : 1;
  // waves per SIMD the register budget is set for: 2 (256 VGPRs), but the fp64 K = 4 instance, whose
  // DPP shifts and selects take two registers per value, fits only the whole file
  static constexpr int WAVES = (K == 4 && sizeof(T) == 8) ? 1 : 2;
};

template <class T, int K, bool RES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Star7Tile<T, K>::WAVES))) void star7_tbk(
    const T* __restrict__ in, T* __restrict__ out, Geo g, sm::Star7W<T> w, int zc, int XT, int YT, int ntasks,
    double* __restrict__ resid) {
  constexpr int N = Star7Tile<T, K>::N, RY = Star7Tile<T, K>::RY;
  using VV = Vec7<T, N>;
  using V = typename VV::type;
  using Row = Row7<T, N>;
  constexpr int OV = (K + N - 1) / N;       // overlap lanes per side
  constexpr int SEG = (64 - 2 * OV) * N;    // owned columns per wave
  constexpr int PD = 2;                     // u0 planes in flight (the plane loop is unrolled by as many)
  constexpr int R0 = RY + 2 * K;            // u0 rows per plane: y0 - K .. y0 + RY + K - 1
  constexpr int TOT = tbk_off<RY, K>(K + 1);  // level rows in all (level l: RY + 2 (K - l))
  const int lane = threadIdx.x & 63;
  // wave-uniform task index in an SGPR, so every row / plane index and test below is scalar
  const int task = (int)xcd_remap(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (task >= ntasks) return;  // wave-uniform; no block barriers in this kernel
  const int xt = task % XT, yt = (task / XT) % YT, zt = task / (XT * YT);
  const int64_t x = (int64_t)xt * SEG - OV * N + (int64_t)lane * N;
  // rows and planes as 32-bit scalars (64-bit compares of wave-uniform values would run on the VALU)
  const int ny = (int)g.ny, gnz = (int)g.gnz, gzo = (int)g.gz_off, lzmax = (int)g.lz_max;
  const int ys = yt * RY;
  const int zs = (int)g.lz_begin + zt * zc;
  const int ze = min((int)g.lz_end, zs + zc);
  const bool own = lane >= OV && lane <= 63 - OV && x >= 0 && x < g.pitch;
  const int64_t plane = g.plane, pitch = g.pitch;
  // per-cell weights: (1, 0, ..., 0) on the held columns
  T k0[N], kxm[N], kxp[N], kym[N], kyp[N], kzm[N], kzp[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const bool held = (x + e <= 0) || (x + e >= g.nx - 1);
    k0[e] = held ? T(1) : w.c0;
    kxm[e] = held ? T(0) : w.xm;
    kxp[e] = held ? T(0) : w.xp;
    kym[e] = held ? T(0) : w.ym;
    kyp[e] = held ? T(0) : w.yp;
    kzm[e] = held ? T(0) : w.zm;
    kzp[e] = held ? T(0) : w.zp;
  }
  // Loads without lane predication: lanes outside the row read the nearest in-row vector, rows outside
  // the plane its nearest row and planes past the storage its nearest plane. Those values are finite
  // and only ever meet held or unowned cells (the left halo lanes of the first segment feed only x = 0,
  // lanes beyond the row only x >= nx - 1 and themselves, rows beyond the plane only the held rows).
  // An address is a wave-uniform 64-bit plane base + a wave-uniform 32-bit row offset (SALU) + the
  // lane's 32-bit byte offset: one VGPR of addressing for all loads, one for all stores.
  const uint32_t xld = (uint32_t)((x < 0 ? 0 : x >= pitch ? pitch - N : x) * (int64_t)sizeof(T));
  const uint32_t xst = (uint32_t)((own ? x : 0) * (int64_t)sizeof(T));
  uint32_t yoff[R0];  // byte offset of u0 row r inside its plane (rows clamped into the plane)
#pragma unroll
  for (int r = 0; r < R0; ++r) {
    const int y = ys - K + r;
    yoff[r] = (uint32_t)((y < 0 ? 0 : y >= ny ? ny - 1 : y) * pitch * (int64_t)sizeof(T));
  }
  auto ld = [&](int lz, int r) -> Row {
    const int lzc = lz < 0 ? 0 : lz >= lzmax ? lzmax - 1 : lz;
    const char* rp = (const char*)in + lzc * plane * (int64_t)sizeof(T) + yoff[r];
    const T* p = (const T*)(rp + xld);
    dcheck(g, in, p, N);
    const V v = *(const V*)p;  // one 8- or 16-B vector
    Row o;
#pragma unroll
    for (int e = 0; e < N; ++e) o.v[e] = VV::get(v, e);
    return o;
  };
  Row P[TOT], C[TOT];  // level l = 1..K, row j at tbk_off(l) + j
#pragma unroll
  for (int i = 0; i < TOT; ++i)
#pragma unroll
    for (int e = 0; e < N; ++e) P[i].v[e] = C[i].v[e] = T(0);
  double acc = 0.0;
  const int qlast = ze - 1 + K;
  // newest u0 plane q; level l finishes plane q - l (each level's first two planes are priming garbage
  // that no level needs). Tasks whose pipeline planes zs - K - 1 .. ze + K and rows ys - K .. ys + RY + K
  // are all interior take the loop copy without the held-row / held-plane test.
  const bool interior = zs - K - 1 + gzo >= 1 && ze + K + gzo <= gnz - 2 && ys - K >= 1 && ys + RY + K <= ny - 1;
  // bit j of yheld[l - 1]: row j of level l is a held row (or lies outside the plane)
  unsigned yheld[K];
#pragma unroll
  for (int l = 1; l <= K; ++l) {
    yheld[l - 1] = 0;
#pragma unroll
    for (int j = 0; j < RY + 2 * (K - l); ++j) {
      const int y = ys - (K - l) + j;
      yheld[l - 1] |= (unsigned)(y <= 0 || y >= ny - 1) << j;
    }
  }
  Row nxr[PD][R0];
#pragma unroll
  for (int i = 0; i < PD; ++i)
#pragma unroll
    for (int r = 0; r < R0; ++r) nxr[i][r] = ld(zs - K + i, r);
  auto plane_step = [&](int q, auto htest, auto slot) __attribute__((always_inline)) {
    constexpr bool HT = decltype(htest)::value;
    constexpr int SL = decltype(slot)::value;  // which in-flight plane is plane q
    Row win[K][3];  // per level m = 0..K-1: its last three rows of this plane (ym, centre, yp of level m + 1)
#pragma unroll
    for (int m = 0; m < K; ++m)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < N; ++e) win[m][i].v[e] = T(0);
#pragma unroll
    for (int r = 0; r < R0; ++r) {
      Row X = nxr[SL][r];  // row rr of level m, starting as row r of u0
      int rr = r;
      bool live = true;
#pragma unroll
      for (int m = 0; m < K; ++m) {
        if (!live) continue;
        win[m][0] = win[m][1];
        win[m][1] = win[m][2];
        win[m][2] = X;
        if (rr < 2) {
          live = false;
          continue;
        }
        // the window is complete for row j of level l
        const int l = m + 1, j = rr - 2, s = tbk_off<RY, K>(l) + j;
        const Row &ym = win[m][0], &c = win[m][1], &yp = win[m][2];
        const int pz = q - l;             // the plane this level finishes
        const int y = ys - (K - l) + j;   // the row
        const int gz = pz + gzo;
        // wave-uniform: a held row or plane is emitted as its centre
        const bool hold = HT && (gz <= 0 || gz >= gnz - 1 || (yheld[m] >> j & 1u));
        const T lft = lane_up1(c.v[N - 1]);
        const T rgt = lane_down1(c.v[0]);
        const Row cold = C[s];
        Row o;
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const T xm = e == 0 ? lft : c.v[e - 1], xp = e == N - 1 ? rgt : c.v[e + 1];
          const T B = sm::star7_B<T>(c.v[e], xm, xp, ym.v[e], yp.v[e], k0[e], kxm[e], kxp[e], kym[e], kyp[e]);
          const T u = sm::star7_finish<T>(P[s].v[e], c.v[e], kzp[e]);
          o.v[e] = hold ? cold.v[e] : u;
          P[s].v[e] = sm::star7_P<T>(B, cold.v[e], kzm[e]);
          C[s].v[e] = c.v[e];
        }
        if (l == K) {
          // (y = ys + j here) store the owned lanes of the chunk's planes
          if (pz >= zs && q <= qlast && y < ny && own) {
            V ov;
#pragma unroll
            for (int e = 0; e < N; ++e) VV::set(ov, e, o.v[e]);
            char* rp = (char*)out + pz * plane * (int64_t)sizeof(T) + (uint32_t)(y * pitch * (int64_t)sizeof(T));
            T* dst = (T*)(rp + xst);
            dcheck(g, (const T*)out, (const T*)dst, N);
            store_nt((V*)dst, ov);
            if (RES) {
#pragma unroll
              for (int e = 0; e < N; ++e)
                if (x + e < g.nx) {
                  const double d = (double)o.v[e] - (double)cold.v[e];
                  acc += d * d;
                }
            }
          }
          live = false;
        } else {
          X = o;
          rr = j;
        }
      }
      // u0 row r - 2 has fed its last level-1 row: its registers take the same row of plane q + PD. The
      // barrier keeps the scheduler from hoisting these loads (a third plane of registers) and from
      // interleaving the rows' chains (their temporaries); the K x N chains of one step stay free.
      if (r >= 2) nxr[SL][r - 2] = ld(q + PD, r - 2);
      __builtin_amdgcn_sched_barrier(0);
    }
    nxr[SL][R0 - 2] = ld(q + PD, R0 - 2);
    nxr[SL][R0 - 1] = ld(q + PD, R0 - 1);
  };
  auto march = [&](auto htest) __attribute__((always_inline)) {
    // an odd plane count ends with one extra plane (q = qlast + 1): loads clamp, nothing is stored
    for (int q = zs - K; q <= qlast; q += 2) {
      plane_step(q, htest, std::integral_constant<int, 0>{});
      plane_step(q + 1, htest, std::integral_constant<int, 1>{});
    }
  };
  if (interior)
    march(std::integral_constant<bool, false>{});
  else
    march(std::integral_constant<bool, true>{});
  if (RES) wave_atomic_add(resid, acc);
}

template <class T>
static sm::Star7W<T> star7_w(const StencilCoef& cf) {
  return sm::Star7W<T>{(T)cf.c0, (T)cf.wxm, (T)cf.wxp, (T)cf.wym, (T)cf.wyp, (T)cf.wzm, (T)cf.wzp};
}

template <class T, int K>
static void launch_star7_k(const Geo& g, const T* in, T* out, const StencilCoef& cf, double* resid, hipStream_t s) {
  const int64_t planes = g.lz_end - g.lz_begin;
  if (planes <= 0) return;
  constexpr int N = Star7Tile<T, K>::N, RY = Star7Tile<T, K>::RY, OV = (K + N - 1) / N, SEG = (64 - 2 * OV) * N;
  MDFX_CHECK(g.ny == g.gny && g.gy_off == 0, "star7_tbk sweeps slab layouts");
  const int XT = (int)((g.nx + SEG - 1) / SEG);
  const int YT = (int)((g.ny + RY - 1) / RY);
  // one to two rounds of resident waves (256 CUs x 8): every chunk re-reads K priming planes per end,
  // so the fused depths take chunks twice as deep as the single step
  const int zc = pick_zc(planes, (int64_t)XT * YT, 128, K == 1 ? 4 * 2048 : 2 * 2048);
  const int64_t ZT = (planes + zc - 1) / zc;
  const int64_t nt = (int64_t)XT * YT * ZT;
  MDFX_CHECK(nt < (int64_t)1 << 30, "star7_tbk: too many tasks for one launch");
  const int ntasks = (int)nt;
  const dim3 grd((unsigned)((ntasks + 3) / 4)), blk(256);
  const sm::Star7W<T> w = star7_w<T>(cf);
  if (resid)
    hipLaunchKernelGGL((star7_tbk<T, K, true>), grd, blk, 0, s, in, out, g, w, zc, XT, YT, ntasks, resid);
  else
    hipLaunchKernelGGL((star7_tbk<T, K, false>), grd, blk, 0, s, in, out, g, w, zc, XT, YT, ntasks, resid);
}

// One cell per lane: the "naive" variant, the on-device oracle of the kernel above (dispatched by
// naive_launch, stencil_naive.hip). It is compiled here so that it shares this file's build flags
// (plain, unpacked fp32 multiplies and fmas). Rows [ly_begin, ly_end) of a pencil's storage, held at
// the GLOBAL y boundary.
template <class T, bool RES>
__global__ __launch_bounds__(256) void naive_star7(const T* __restrict__ in, T* __restrict__ out, Geo g,
                                                   sm::Star7W<T> w, double* __restrict__ resid) {
  const int64_t nr = g.ly_end - g.ly_begin;
  const int64_t n = g.nx * nr * (g.lz_end - g.lz_begin);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t x = i % g.nx, t = i / g.nx, y = g.ly_begin + t % nr, lz = g.lz_begin + t / nr;
    const int64_t gz = lz + g.gz_off, gy = y + g.gy_off;
    const int64_t idx = lz * g.plane + y * g.pitch + x;
    const T c = in[idx];
    T o = c;
    if (x > 0 && x < g.nx - 1 && gy > 0 && gy < g.gny - 1 && gz > 0 && gz < g.gnz - 1)
      o = sm::star7<T>(c, in[idx - 1], in[idx + 1], in[idx - g.pitch], in[idx + g.pitch], in[idx - g.plane],
                       in[idx + g.plane], w);
    out[idx] = o;
    if (RES) {
      const double d = (double)o - (double)c;
      acc += d * d;
    }
  }
  if (RES) wave_atomic_add(resid, acc);
}

template <class T>
void launch_star7_naive(const Geo& g, const T* in, T* out, const StencilCoef& cf, double* resid, hipStream_t s) {
  const int64_t n = g.nx * (g.ly_end - g.ly_begin) * (g.lz_end - g.lz_begin);
  if (n <= 0) return;
  const dim3 grd((unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32)), blk(256);
  const sm::Star7W<T> w = star7_w<T>(cf);
  if (resid)
    hipLaunchKernelGGL((naive_star7<T, true>), grd, blk, 0, s, in, out, g, w, resid);
  else
    hipLaunchKernelGGL((naive_star7<T, false>), grd, blk, 0, s, in, out, g, w, resid);
}
template void launch_star7_naive<float>(const Geo&, const float*, float*, const StencilCoef&, double*, hipStream_t);
template void launch_star7_naive<double>(const Geo&, const double*, double*, const StencilCoef&, double*, hipStream_t);

// steps = 1 or one of the fused depths 2, 3, 4 (hip_supports_steps)
template <class T>
void launch_star7(const Geo& g, const T* in, T* out, const StencilCoef& cf, int steps, double* resid, hipStream_t s) {
  switch (steps) {
    case 1: launch_star7_k<T, 1>(g, in, out, cf, resid, s); break;
    case 2: launch_star7_k<T, 2>(g, in, out, cf, resid, s); break;
    case 3: launch_star7_k<T, 3>(g, in, out, cf, resid, s); break;
    case 4: launch_star7_k<T, 4>(g, in, out, cf, resid, s); break;
    default: MDFX_FAIL(format("no star7 kernel fuses %d steps (1, 2, 3, 4)", steps));
  }
}
template void launch_star7<float>(const Geo&, const float*, float*, const StencilCoef&, int, double*, hipStream_t);
template void launch_star7<double>(const Geo&, const double*, double*, const StencilCoef&, int, double*, hipStream_t);

}  // namespace dev
}  // namespace mdfx
