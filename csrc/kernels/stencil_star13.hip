// 3D radius-2 star (star13), the fourth-order Laplacian's 13 points:
//   u' = c0*u + c1*(the 6 neighbours at distance 1) + c2*(the 6 neighbours at distance 2 along the axes),
// one step (the K = 1 instance) or K = 2 fused steps per sweep over memory (star13_tbk).
//
// Arithmetic (sm::star13_B / star13_P / star13_zp1 / star13_zp2, shared with the CPU oracle and the naive
// kernel): one multiply and twelve fmas, ordered for the z march. B is the cell's own plane (centre, x-1,
// x+1, x-2, x+2, y-1, y+1, y-2, y+2), P adds z-2 and z-1 and is final the moment plane z has arrived, and
// the planes z+1 and z+2 add one fma each as they arrive. There are no adds, so nothing can be contracted
// differently on host and device.
//
// How the work is split: every wave is an independent task; no LDS, no block barrier (a block is four
// tasks). The y window goes through registers, not LDS: a radius-2 window in LDS would need the plane of
// every fused level written and read back behind two block barriers per plane, while a wave that owns
// its rows keeps the whole K-level pipeline in one instruction stream. The price is the trapezoid: 4
// redundant rows per fused level. A task is
//   - an x segment of 64 lanes x N cells (16 B per lane, fp32 fused 8 B: N = 4 / 2 fp32, 2 fp64). With
//     N >= 2 both x neighbours of a side lie in the adjacent lane, so two DPP shifts per side serve both
//     distances. OV = ceil(2K / N) overlap lanes per side: a wave owns (and stores) only lanes
//     OV .. 63 - OV. The outermost lane of a wave sees 0 instead of its neighbours and every level
//     corrupts two more columns from outside; after 2K <= OV * N columns the owned lanes are still exact;
//   - a y strip of RY output rows, handled as a trapezoid inside the wave: u0 arrives in RY + 4K rows
//     and level l computes the RY + 4(K - l) rows y0 - 2(K - l) .. y0 + RY + 2(K - l) - 1;
//   - a chunk of zc planes to march over (+ 2K priming planes at each end).
//
// What a level holds, per row, once plane p of its input has arrived: the centres C1 = c(p), C2 = c(p-1),
// S1 = P(p) (waits for p+1, p+2) and S2 = fma(c1, c(p), P(p-1)) (waits for p+1). The arriving plane
// p + 1 with centre c finishes u(p-1) = fma(c2, c, S2), hands it to the next level and rolls
// S2 = fma(c1, c, S1), S1 = P(p+1) from its own 5-row window, C2 = C1, C1 = c. So level l emits plane
// q - 2l when plane q of u0 arrives, and an arriving u0 row cascades through all K levels: row r of level
// l - 1 completes the 5-row window of row r - 4 of level l. Everything is unrolled, so the windows are
// register names. A u0 row's registers are reloaded with the same row of plane q + 1 the moment the row
// leaves the first level's window: one plane of u0 in flight.
//
// Held cells (any coordinate within 2 of a global face) are an exact select of the centre C2: per lane
// for the columns, wave-uniform for rows and planes. Only the loop copy for tasks that touch the frame
// carries the select; tasks whose lanes, rows and pipeline planes are all free run a copy without it.
// Loads are not lane-predicated but clamped into the row, the plane and the storage; what a clamped load
// returns only ever meets held or unowned cells.
//
// What is stored: level K's rows of the planes zs .. ze - 1 of the chunk, owned lanes only, non-temporal.
//
// Region contract: output storage planes [lz_begin, lz_end) need u0 valid on [lz_begin - 2K, lz_end + 2K).
// Slab geometry only.
#include <algorithm>
#include <type_traits>

#include "kcommon.hpp"
#include "launchers.hpp"
#include "mdfx/kernels.hpp"
#include "mdfx/stencil_math.hpp"

namespace mdfx {
namespace dev {

template <class T, int N>
struct Row13 {
  T v[N];
};

// first row of level l (1..K) in the flat per-level state arrays (level l has RY + 4 (K - l) rows)
template <int RY, int K>
__host__ __device__ constexpr int s13_off(int l) {
  return (l - 1) * RY + 4 * ((l - 1) * K - (l - 1) * l / 2);
}

// Tile constants per (T, K). A level row costs 4 values (S1, S2, C1, C2) x N x sizeof(T) / 4 registers,
// the u0 plane in flight RY + 4K rows. K = 1: strips of 4 rows, 2 waves per SIMD (182 VGPRs). K = 2: the
// fp32 rows are 8 B per lane so that the 4 + 8 level rows of a 4-row strip fit 2 waves per SIMD (223
// VGPRs); fp64 needs 16 B per lane to keep the x neighbours in the adjacent lane, and its level rows fit
// only the whole register file (one wave per SIMD) in strips of 3 (366 VGPRs + 104 AGPRs; strips of 4
// took 428 + 172). Row-update redundancy of K = 2, (RY + 4 + RY) / 2 RY: 1.5 fp32, 1.67 fp64. No scratch.
template <class T, int K>
struct Star13Tile {
  static constexpr int N = (K == 1 || sizeof(T) == 8) ? 16 / (int)sizeof(T) : 2;
  static constexpr int RY = (K == 2 && sizeof(T) == 8) ? 3 : 4;
  static constexpr int WAVES = (K == 2 && sizeof(T) == 8) ? 1 : 2;
};

template <class T, int K, bool RES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Star13Tile<T, K>::WAVES))) void star13_tbk(
    const T* __restrict__ in, T* __restrict__ out, Geo g, sm::Star13W<T> w, int zc, int XT, int YT, int ntasks,
    double* __restrict__ resid) {
  constexpr int N = Star13Tile<T, K>::N, RY = Star13Tile<T, K>::RY;
  typedef T V __attribute__((ext_vector_type(N)));
  using Row = Row13<T, N>;
  static_assert(N >= 2, "both x neighbours of a side must lie in the adjacent lane");
  constexpr int OV = (2 * K + N - 1) / N;     // overlap lanes per side
  constexpr int SEG = (64 - 2 * OV) * N;      // owned columns per wave
  constexpr int R0 = RY + 4 * K;              // u0 rows per plane: y0 - 2K .. y0 + RY + 2K - 1
  constexpr int TOT = s13_off<RY, K>(K + 1);  // level rows in all
  const int lane = threadIdx.x & 63;
  // wave-uniform task index in an SGPR, so every row / plane index and test below is scalar
  const int task = (int)xcd_remap(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (task >= ntasks) return;  // wave-uniform; no block barriers in this kernel
  const int xt = task % XT, yt = (task / XT) % YT, zt = task / (XT * YT);
  const int xw = xt * SEG - OV * N;  // the wave's first column (lane 0)
  const int64_t x = (int64_t)xw + (int64_t)lane * N;
  const int nx = (int)g.nx, ny = (int)g.ny, gnz = (int)g.gnz, gzo = (int)g.gz_off, lzmax = (int)g.lz_max;
  const int ys = yt * RY;
  const int zs = (int)g.lz_begin + zt * zc;
  const int ze = min((int)g.lz_end, zs + zc);
  const bool own = lane >= OV && lane <= 63 - OV && x >= 0 && x < g.pitch;
  const int64_t plane = g.plane, pitch = g.pitch;
  // held columns (the pad beyond the row included: it is copied through)
  bool hx[N];
#pragma unroll
  for (int e = 0; e < N; ++e) hx[e] = (x + e < 2) || (x + e >= nx - 2);
  // An address is a wave-uniform 64-bit plane base + a wave-uniform 32-bit row offset (SALU) + the
  // lane's 32-bit byte offset: one VGPR of addressing for all loads, one for all stores.
  const uint32_t xld = (uint32_t)((x < 0 ? 0 : x >= pitch ? pitch - N : x) * (int64_t)sizeof(T));
  const uint32_t xst = (uint32_t)((own ? x : 0) * (int64_t)sizeof(T));
  uint32_t yoff[R0];  // byte offset of u0 row r inside its plane (rows clamped into the plane)
#pragma unroll
  for (int r = 0; r < R0; ++r) {
    const int y = ys - 2 * K + r;
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
    for (int e = 0; e < N; ++e) o.v[e] = v[e];
    return o;
  };
  Row S1[TOT], S2[TOT], C1[TOT], C2[TOT];  // level l = 1..K, row j at s13_off(l) + j
#pragma unroll
  for (int i = 0; i < TOT; ++i)
#pragma unroll
    for (int e = 0; e < N; ++e) S1[i].v[e] = S2[i].v[e] = C1[i].v[e] = C2[i].v[e] = T(0);
  double acc = 0.0;
  const int q0 = zs - 2 * K, qlast = ze - 1 + 2 * K;
  // newest u0 plane q; level l finishes plane q - 2l (each level's first four planes are priming garbage
  // that no level needs). Tasks whose lanes, rows ys - 2K .. ys + RY + 2K and pipeline planes are all
  // free take the loop copy without the held-cell select.
  const bool interior = xw >= 2 && xw + 64 * N <= nx - 2 && ys - 2 * K >= 2 && ys + RY + 2 * K <= ny - 2 &&
                        q0 - 2 + gzo >= 2 && qlast + gzo <= gnz - 3;
  // bit j of yheld[l - 1]: row j of level l is a held row (or lies outside the plane)
  unsigned yheld[K];
#pragma unroll
  for (int l = 1; l <= K; ++l) {
    yheld[l - 1] = 0;
#pragma unroll
    for (int j = 0; j < RY + 4 * (K - l); ++j) {
      const int y = ys - 2 * (K - l) + j;
      yheld[l - 1] |= (unsigned)(y < 2 || y >= ny - 2) << j;
    }
  }
  Row nxr[R0];
#pragma unroll
  for (int r = 0; r < R0; ++r) nxr[r] = ld(q0, r);
  auto plane_step = [&](int q, auto htest) __attribute__((always_inline)) {
    constexpr bool HT = decltype(htest)::value;
    Row win[K][5];  // per level m = 0..K-1: its last five rows of this plane (the y window of level m + 1)
#pragma unroll
    for (int m = 0; m < K; ++m)
#pragma unroll
      for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int e = 0; e < N; ++e) win[m][i].v[e] = T(0);
#pragma unroll
    for (int r = 0; r < R0; ++r) {
      Row X = nxr[r];  // row rr of level m, starting as row r of u0
      int rr = r;
      bool live = true;
#pragma unroll
      for (int m = 0; m < K; ++m) {
        if (!live) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) win[m][i] = win[m][i + 1];
        win[m][4] = X;
        if (rr < 4) {
          live = false;
          continue;
        }
        // the window is complete for row j of level l
        const int l = m + 1, j = rr - 4, s = s13_off<RY, K>(l) + j;
        const Row &ym2 = win[m][0], &ym1 = win[m][1], &c = win[m][2], &yp1 = win[m][3], &yp2 = win[m][4];
        const int pz = q - 2 * l;               // the plane this level finishes
        const int y = ys - 2 * (K - l) + j;     // the row
        const int gz = pz + gzo;
        // wave-uniform: a held row or plane is emitted as its centre
        const bool hold = HT && (gz < 2 || gz >= gnz - 2 || (yheld[m] >> j & 1u));
        // the adjacent lanes' two nearest cells
        const T l1 = lane_up1(c.v[N - 1]), l2 = lane_up1(c.v[N - 2]);
        const T r1 = lane_down1(c.v[0]), r2 = lane_down1(c.v[1]);
        const Row cold = C2[s];  // the centre of the plane being finished
        Row o;
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const T xm1 = e >= 1 ? c.v[e >= 1 ? e - 1 : 0] : l1;
          const T xm2 = e >= 2 ? c.v[e >= 2 ? e - 2 : 0] : e == 1 ? l1 : l2;
          const T xp1 = e <= N - 2 ? c.v[e <= N - 2 ? e + 1 : 0] : r1;
          const T xp2 = e <= N - 3 ? c.v[e <= N - 3 ? e + 2 : 0] : e == N - 2 ? r1 : r2;
          const T B = sm::star13_B<T>(c.v[e], xm1, xp1, xm2, xp2, ym1.v[e], yp1.v[e], ym2.v[e], yp2.v[e], w);
          const T u = sm::star13_zp2<T>(S2[s].v[e], c.v[e], w);
          o.v[e] = (HT && (hold || hx[e])) ? cold.v[e] : u;
          S2[s].v[e] = sm::star13_zp1<T>(S1[s].v[e], c.v[e], w);
          S1[s].v[e] = sm::star13_P<T>(B, cold.v[e], C1[s].v[e], w);
          C2[s].v[e] = C1[s].v[e];
          C1[s].v[e] = c.v[e];
        }
        if (l == K) {
          // (y = ys + j here) store the owned lanes of the chunk's planes
          if (pz >= zs && pz < ze && y < ny && own) {
            V ov;
#pragma unroll
            for (int e = 0; e < N; ++e) ov[e] = o.v[e];
            char* rp = (char*)out + pz * plane * (int64_t)sizeof(T) + (uint32_t)(y * pitch * (int64_t)sizeof(T));
            T* dst = (T*)(rp + xst);
            dcheck(g, (const T*)out, (const T*)dst, N);
            store_nt((V*)dst, ov);
            if (RES) {
#pragma unroll
              for (int e = 0; e < N; ++e)
                if (x + e < nx) {
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
      // u0 row r - 4 has left the first level's window: its registers take the same row of plane q + 1.
      // The barrier keeps the scheduler from hoisting these loads (a second plane of registers) and from
      // interleaving the rows' chains (their temporaries); the N chains of one row stay free.
      if (r >= 4) nxr[r - 4] = ld(q + 1, r - 4);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int r = R0 - 4; r < R0; ++r) nxr[r] = ld(q + 1, r);
  };
  if (interior) {
    for (int q = q0; q <= qlast; ++q) plane_step(q, std::integral_constant<bool, false>{});
  } else {
    for (int q = q0; q <= qlast; ++q) plane_step(q, std::integral_constant<bool, true>{});
  }
  if (RES) wave_atomic_add(resid, acc);
}

template <class T>
static sm::Star13W<T> star13_w(const StencilCoef& cf) {
  return sm::Star13W<T>{(T)cf.c0, (T)cf.c1, (T)cf.c2};
}

template <class T, int K>
static void launch_star13_k(const Geo& g, const T* in, T* out, const StencilCoef& cf, double* resid, hipStream_t s) {
  const int64_t planes = g.lz_end - g.lz_begin;
  if (planes <= 0) return;
  constexpr int N = Star13Tile<T, K>::N, RY = Star13Tile<T, K>::RY, OV = (2 * K + N - 1) / N, SEG = (64 - 2 * OV) * N;
  MDFX_CHECK(g.ny == g.gny && g.gy_off == 0, "star13_tbk sweeps slab layouts");
  MDFX_CHECK(g.nx < ((int64_t)1 << 30) && g.ny < ((int64_t)1 << 30) && g.lz_max < ((int64_t)1 << 30) &&
                 g.plane * (int64_t)sizeof(T) < ((int64_t)1 << 32),
             "star13_tbk: 32-bit row, plane and in-plane byte offsets");
  const int XT = (int)((g.nx + SEG - 1) / SEG);
  const int YT = (int)((g.ny + RY - 1) / RY);
  // one to two rounds of resident waves (256 CUs x 8): every chunk re-reads 2K priming planes per end,
  // so the fused depth takes chunks twice as deep as the single step
  const int zc = pick_zc(planes, (int64_t)XT * YT, 128, K == 1 ? 4 * 2048 : 2 * 2048);
  const int64_t ZT = (planes + zc - 1) / zc;
  const int64_t nt = (int64_t)XT * YT * ZT;
  MDFX_CHECK(nt < (int64_t)1 << 30, "star13_tbk: too many tasks for one launch");
  const int ntasks = (int)nt;
  const dim3 grd((unsigned)((ntasks + 3) / 4)), blk(256);
  const sm::Star13W<T> w = star13_w<T>(cf);
  if (resid)
    hipLaunchKernelGGL((star13_tbk<T, K, true>), grd, blk, 0, s, in, out, g, w, zc, XT, YT, ntasks, resid);
  else
    hipLaunchKernelGGL((star13_tbk<T, K, false>), grd, blk, 0, s, in, out, g, w, zc, XT, YT, ntasks, resid);
}

// One cell per lane: the "naive" variant, the on-device oracle of the kernel above (dispatched by
// naive_launch, stencil_naive.hip). It is compiled here so that it shares this file's build flags
// (plain, unpacked fp32 multiplies and fmas). A cell within 2 of a global face is copied through, so no
// neighbour index leaves the grid.
template <class T, bool RES>
__global__ __launch_bounds__(256) void naive_star13(const T* __restrict__ in, T* __restrict__ out, Geo g,
                                                    sm::Star13W<T> w, double* __restrict__ resid) {
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
    if (x >= 2 && x < g.nx - 2 && gy >= 2 && gy < g.gny - 2 && gz >= 2 && gz < g.gnz - 2)
      o = sm::star13<T>(c, in[idx - 1], in[idx + 1], in[idx - 2], in[idx + 2], in[idx - g.pitch], in[idx + g.pitch],
                        in[idx - 2 * g.pitch], in[idx + 2 * g.pitch], in[idx - 2 * g.plane], in[idx - g.plane],
                        in[idx + g.plane], in[idx + 2 * g.plane], w);
    out[idx] = o;
    if (RES) {
      const double d = (double)o - (double)c;
      acc += d * d;
    }
  }
  if (RES) wave_atomic_add(resid, acc);
}

template <class T>
void launch_star13_naive(const Geo& g, const T* in, T* out, const StencilCoef& cf, double* resid, hipStream_t s) {
  const int64_t n = g.nx * (g.ly_end - g.ly_begin) * (g.lz_end - g.lz_begin);
  if (n <= 0) return;
  const dim3 grd((unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32)), blk(256);
  const sm::Star13W<T> w = star13_w<T>(cf);
  if (resid)
    hipLaunchKernelGGL((naive_star13<T, true>), grd, blk, 0, s, in, out, g, w, resid);
  else
    hipLaunchKernelGGL((naive_star13<T, false>), grd, blk, 0, s, in, out, g, w, resid);
}
template void launch_star13_naive<float>(const Geo&, const float*, float*, const StencilCoef&, double*, hipStream_t);
template void launch_star13_naive<double>(const Geo&, const double*, double*, const StencilCoef&, double*, hipStream_t);

// steps = 1 or the fused depth 2 (hip_supports_steps)
template <class T>
void launch_star13(const Geo& g, const T* in, T* out, const StencilCoef& cf, int steps, double* resid, hipStream_t s) {
  switch (steps) {
    case 1: launch_star13_k<T, 1>(g, in, out, cf, resid, s); break;
    case 2: launch_star13_k<T, 2>(g, in, out, cf, resid, s); break;
    default: MDFX_FAIL(format("no star13 kernel fuses %d steps (1, 2)", steps));
  }
}
template void launch_star13<float>(const Geo&, const float*, float*, const StencilCoef&, int, double*, hipStream_t);
template void launch_star13<double>(const Geo&, const double*, double*, const StencilCoef&, int, double*, hipStream_t);

}  // namespace dev
}  // namespace mdfx
