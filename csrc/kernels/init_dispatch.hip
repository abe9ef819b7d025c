// Device-side field initialisation and the stencil dispatcher (variant selection + geometry).
//
// Reference parity: create_universe (MDF_kernel.cu:88-99, kernel.cu:131-146) built the grid on the
// host and shipped it over PCIe every generation (D12); here the initial condition is generated
// in place on the device from the *global* cell index, so every decomposition yields the same grid
// and no host copy is needed.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "kcommon.hpp"
#include "launchers.hpp"
#include "mdfx/kernels.hpp"

namespace mdfx {
namespace dev {

// 3D 7-point sweeps of K >= 3 steps run heat7_wtk (wave-independent tiles; 1024^3 fp32 K = 3:
// 1443 vs 1081 GCells/s for heat7_tbk, profiles/archive/r02_wtk/README.txt; heat7_tbk's K = 3 / 4 were
// removed in round 5)
static bool use_wxk(DType dt, int64_t nx, int steps);
// (fp32 K = 5: heat7_wxk only, in rows of 2 cells per lane)
static bool use_wtk(int steps, DType dt) {
  return heat7_wtk_supported(steps) || ((dt == DType::F32 || dt == DType::F64) && steps == 5);
}
// ... and among them heat7_wxk (y halo exchanged inside the band, stencil_heat_wxk.hip) for fp32:
// 1024^3 K = 4 2262 GCells/s vs heat7_wtk K = 3 1868 on one box (profiles/archive/r03_wxk/); since
// round 6 heat7_wtk is fp64 only (its fp32 instances ran only under MDFX_H7_WXK=0: 12 kernels,
// ~290 KB of code object, removed). MDFX_H7_WXK = 0 / 1 forces fp64's choice off / on. fp64 K = 3
// takes it from 2048-cell rows on, in 3 + 1-row bands: 2048^3
// fp64 + residual every 12 897 vs 796 GCells/s for heat7_wtk, while at 1024-cell rows heat7_wtk's
// 3-row waves stay ahead (907 vs 874) (profiles/archive/r03_session_p/). fp64 K = 4 always runs it, in
// 2 + 1-row bands (heat7_wtk's K = 4 needs 1-row waves: 1024^3 1112-1124 vs 418 GCells/s,
// profiles/r04_session_o/)
static bool use_wxk(DType dt, int64_t nx, int steps) {
  return steps >= 5 || dt == DType::F32 || knobs().h7_wxk == 1 || (knobs().h7_wxk < 0 && (nx >= 2048 || steps == 4));
}

static int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  if (!v || !*v) return dflt;
  return std::atoi(v);
}

static Knobs read_knobs() {
  Knobs k;
  k.tb_ry = env_int("MDFX_TB_RY", 0);
  k.wtk_wb = env_int("MDFX_WTK_WB", 0);
  k.h7_wxk = env_int("MDFX_H7_WXK", -1);
  k.b27_wxk = env_int("MDFX_B27_WXK", -1);
  k.devcheck_selftest = env_int("MDFX_DEVCHECK_SELFTEST", 0);
  k.fold_release = env_int("MDFX_FOLD_RELEASE", 0);
  return k;
}

// Published snapshots are never freed (a launch on another thread may still read the previous
// one); a reload allocates a few dozen bytes.
static std::atomic<const Knobs*> g_knobs{nullptr};

const Knobs& knobs() {
  const Knobs* k = g_knobs.load(std::memory_order_acquire);
  if (!k) {
    hip_reload_knobs();
    k = g_knobs.load(std::memory_order_acquire);
  }
  return *k;
}

struct InitArgs {
  int kind;
  uint64_t seed;
  double lo, hi, value, edge, interior, density;
  int dims;
};

template <class T>
__global__ __launch_bounds__(256) void init_kernel(T* __restrict__ buf, Geo g, InitArgs a) {
  const int64_t n = g.pitch * g.ny * g.lz_max;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t x = i % g.pitch, t = i / g.pitch, y = t % g.ny, lz = t / g.ny;
    const int64_t gz = lz + g.gz_off, gy = y + g.gy_off;  // (a pencil's ghost rows beyond the grid stay 0)
    double v = 0.0;
    if (x < g.nx && gz >= 0 && gz < g.gnz && gy >= 0 && gy < g.gny) {
      const bool bnd = x == 0 || x == g.nx - 1 || gz == 0 || gz == g.gnz - 1 ||
                       (a.dims == 3 && (gy == 0 || gy == g.gny - 1));
      const uint64_t gidx = (uint64_t)x + (uint64_t)g.nx * ((uint64_t)gy + (uint64_t)g.gny * (uint64_t)gz);
      switch (a.kind) {
        case 0: v = a.value; break;
        case 1: v = bnd ? a.edge : a.interior; break;
        case 2: v = fma(a.hi - a.lo, hash_unit(a.seed, gidx), a.lo); break;
        default: v = (!bnd && hash_unit(a.seed, gidx) < a.density) ? 1.0 : 0.0; break;
      }
    }
    buf[lz * g.plane + y * g.pitch + x] = (T)v;
  }
}

#ifdef MDFX_DEVICE_CHECKS
// one violation counter per device (make devcheck builds only)
static std::mutex g_oob_mu;
static std::map<int, unsigned long long*> g_oob;
static unsigned long long* oob_counter() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_oob_mu);
  auto it = g_oob.find(dev);
  if (it != g_oob.end()) return it->second;
  void* p = nullptr;
  if (hipMalloc(&p, sizeof(unsigned long long)) != hipSuccess) return nullptr;
  if (hipMemset(p, 0, sizeof(unsigned long long)) != hipSuccess) return nullptr;
  return g_oob[dev] = (unsigned long long*)p;
}
#endif

static Geo make_geo(const FieldLayout& lay, int64_t lz_begin, int64_t lz_end) {
  Geo g;
  g.alloc = lay.elems() + kSlackBytes / (int64_t)lay.esize();
#ifdef MDFX_DEVICE_CHECKS
  g.oob = oob_counter();
  // self-test of the checking machinery: pretend the allocation is half its size so in-bounds
  // accesses beyond that count as violations (nothing is accessed out of bounds)
  if (knobs().devcheck_selftest) g.alloc = lay.elems() / 2;
#endif
  g.pitch = lay.pitch;
  g.plane = lay.plane;
  g.nx = lay.global.nx;
  g.ny = lay.rows();
  g.gny = lay.global.ny;
  g.gy_off = lay.y0 - lay.hy;
  g.ly_begin = lay.hy;
  g.ly_end = lay.hy + lay.nyl();
  g.gnz = lay.global.nz;
  g.lz_begin = lz_begin;
  g.lz_end = lz_end;
  g.gz_off = lay.z0 - lay.halo;
  g.lz_max = lay.planes();
  return g;
}

static std::mutex g_variant_mu;
static std::string g_variant = "auto";

// The launcher families of launchers.hpp; None: no kernel serves the request.
enum class Kernel {
  None, Naive, Heat7Zw, Heat7Tb2, Heat7Tbk, Heat7Wtk, Heat7Wxk, Box27Zw, Box27Tb2, Box27Wxk, Jacobi5Wave, Jacobi5Tb2,
  Jacobi5Tbk, Box9, Conv9, Star7, Star13, LifeWave, LifeTb2, LifeTbk, LifeRule, LifeGen
};

static const char* kernel_name(Kernel k) {
  static const char* const names[] = {
      "", "naive", "heat7_zw", "heat7_tb2", "heat7_tbk", "heat7_wtk", "heat7_wxk", "box27_zw", "box27_tb2", "box27_wxk",
      "jacobi5_wave", "jacobi5_tb2", "jacobi5_tbk", "box9_tbk", "conv9_tbk", "star7_tbk", "star13_tbk", "life_wave",
      "life_tb2", "life_bits", "life_rule_bits", "life_gen_bits"};
  static_assert(sizeof(names) / sizeof(*names) == (size_t)Kernel::LifeGen + 1, "one name per Kernel, in its order");
  return names[(int)k];
}

struct Choice {
  Kernel kernel;  // what a one-region launch runs
  bool pair;      // two regions go out as one launch (else one after the other)
  bool signals;   // the kernel honours RegionArgs::sig
};

// Which kernel serves (stencil, dtype, layout, steps): the one place that decides it. hip_supports_steps,
// hip_region_signals, hip_kernel_name and the launch in hip_stencil all read this answer.
static Choice choose(const StencilSpec& spec, const FieldLayout& lay, int steps) {
  const auto one = [](Kernel k) { return Choice{k, false, false}; };
  if (steps == 1) {
    // pencil layouts: single steps through the one-cell-per-lane kernels (every stencil); the tuned
    // kernels but heat7_wxk assume slab geometry
    bool naive = lay.pencil();
    if (!naive) {
      std::lock_guard<std::mutex> lk(g_variant_mu);
      naive = g_variant == "naive";
    }
    if (naive) return one(Kernel::Naive);
    switch (spec.kind) {
      case StencilKind::Heat7: return one(Kernel::Heat7Zw);
      case StencilKind::Jacobi5: return one(Kernel::Jacobi5Wave);
      case StencilKind::Box27: return one(Kernel::Box27Zw);
      case StencilKind::Box9: return one(Kernel::Box9);
      case StencilKind::Conv9: return one(Kernel::Conv9);
      case StencilKind::Star7: return one(Kernel::Star7);
      case StencilKind::Star13: return one(Kernel::Star13);
      case StencilKind::Life:
        // a Generations rule of more than 32 states has the naive single step only
        if (spec.generations()) return one(life_gen_supported(spec.coef.states, 1) ? Kernel::LifeGen : Kernel::Naive);
        return one(spec.conway() ? Kernel::LifeWave : Kernel::LifeRule);
    }
    return one(Kernel::None);
  }
  if (steps < 2 || lay.halo < stencil_radius(spec.kind) * steps) return one(Kernel::None);
  if (lay.pencil()) {
    // pencils (y ghost rows): the fused 7-point sweep of heat7_wxk only; two regions go out as one
    // launch where a slab of these rows would run heat7_wxk too
    if (spec.kind == StencilKind::Heat7 && heat7_wxk_supported(steps) && lay.hy >= steps && knobs().h7_wxk != 0)
      return {Kernel::Heat7Wxk, use_wxk(spec.dtype, lay.global.nx, steps), false};
    return one(Kernel::None);
  }
  const bool k2d = steps == 2 || steps == 3 || steps == 4 || steps == 6 || steps == 8;
  switch (spec.kind) {
    case StencilKind::Jacobi5:  // deep temporal blocking of the 2D problems
      if (!((spec.dtype == DType::F32 || spec.dtype == DType::F64) && k2d)) return one(Kernel::None);
      // ref_precision takes the mixed kernels (jacobi5_tbk REF) only where it can change a bit (mixed_update())
      return one(steps > 2 || spec.mixed_update() ? Kernel::Jacobi5Tbk : Kernel::Jacobi5Tb2);
    case StencilKind::Box9: return one(k2d ? Kernel::Box9 : Kernel::None);
    case StencilKind::Conv9: return one(k2d ? Kernel::Conv9 : Kernel::None);
    case StencilKind::Star7: return one(steps <= 4 ? Kernel::Star7 : Kernel::None);    // any nx, ny, nz
    case StencilKind::Star13: return one(steps == 2 ? Kernel::Star13 : Kernel::None);  // any nx, ny, nz
    case StencilKind::Life:
      // a Generations rule: life_gen_bits' depths for 3 .. 32 states; more states have the naive single step only
      if (spec.generations()) return one(life_gen_supported(spec.coef.states, steps) ? Kernel::LifeGen : Kernel::None);
      // 12 / 16: life_bits; the same depths for every other rule through life_rule_bits
      if (!(k2d || steps == 12 || steps == 16)) return one(Kernel::None);
      if (!spec.conway()) return one(Kernel::LifeRule);
      return one(steps > 2 ? Kernel::LifeTbk : Kernel::LifeTb2);
    case StencilKind::Box27: {
      if (steps == 3) return {Kernel::Box27Wxk, true, false};  // (any row width)
      bool tb2 = false;
      const Geo g = make_geo(lay, lay.halo, lay.halo + lay.nzl());
      MDFX_BY_DTYPE(spec.dtype, nullptr, nullptr, tb2 = steps == 2 && box27_tb2_supported<T>(g));
      return one(tb2 ? Kernel::Box27Tb2 : Kernel::None);
    }
    case StencilKind::Heat7: {
      if (use_wtk(steps, spec.dtype)) {
        if (use_wxk(spec.dtype, lay.global.nx, steps)) return {Kernel::Heat7Wxk, true, true};
        return one(Kernel::Heat7Wtk);  // (fp64 only: use_wxk holds for every fp32 sweep)
      }
      // rows within one block: the streaming K-step kernel; wider rows (K = 2): heat7_tb2 x tiles
      bool tbk = false, tb2 = false;
      const Geo g = make_geo(lay, lay.halo, lay.halo + lay.nzl());
      MDFX_BY_DTYPE(spec.dtype, nullptr, nullptr, tbk = heat7_tbk_supported<T>(g, steps);
                    tb2 = steps == 2 && heat7_tb2_supported<T>(g));
      return one(tbk ? Kernel::Heat7Tbk : tb2 ? Kernel::Heat7Tb2 : Kernel::None);
    }
  }
  return one(Kernel::None);
}

}  // namespace dev

int64_t hip_device_check_violations() {
#ifdef MDFX_DEVICE_CHECKS
  int64_t total = 0;
  std::lock_guard<std::mutex> lk(dev::g_oob_mu);
  for (auto& kv : dev::g_oob) {
    unsigned long long h = 0;
    if (hipSetDevice(kv.first) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(&h, kv.second, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
      MDFX_FAIL("reading the device-check counter failed");
    total += (int64_t)h;
  }
  return total;
#else
  return -1;
#endif
}

int hip_runtime_version() {
  int v = 0;
  return hipRuntimeGetVersion(&v) == hipSuccess ? v : 0;
}

void hip_reload_knobs() {
  dev::g_knobs.store(new dev::Knobs(dev::read_knobs()), std::memory_order_release);
}

void hip_set_kernel_variant(const char* name) {
  std::lock_guard<std::mutex> lk(dev::g_variant_mu);
  const std::string v = name ? name : "auto";
  MDFX_CHECK(v == "auto" || v == "naive" || v == "tuned", "unknown kernel variant " + v);
  dev::g_variant = v;
}

const char* hip_kernel_variant() {
  std::lock_guard<std::mutex> lk(dev::g_variant_mu);
  return dev::g_variant.c_str();
}

void hip_init(const InitSpec& init, const FieldLayout& lay, void* buf, void* stream) {
  const dev::Geo g = dev::make_geo(lay, 0, lay.planes());
  dev::InitArgs a{(int)init.kind, init.seed, init.lo,       init.hi,  init.value,
                  init.edge,      init.interior, init.density, lay.global.ny == 1 ? 2 : 3};
  const int64_t n = lay.pitch * lay.rows() * lay.planes();
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 256 * 64);
  hipStream_t s = (hipStream_t)stream;
  switch (lay.dtype) {
    case DType::F32:
      hipLaunchKernelGGL(dev::init_kernel<float>, dim3(grid), dim3(256), 0, s, (float*)buf, g, a);
      break;
    case DType::F64:
      hipLaunchKernelGGL(dev::init_kernel<double>, dim3(grid), dim3(256), 0, s, (double*)buf, g, a);
      break;
    case DType::U8:
      hipLaunchKernelGGL(dev::init_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, (uint8_t*)buf, g, a);
      break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) MDFX_FAIL(std::string("init launch failed: ") + hipGetErrorString(e));
}

bool hip_supports_steps(const StencilSpec& spec, const FieldLayout& lay, int steps) {
  return dev::choose(spec, lay, steps).kernel != dev::Kernel::None;
}

bool hip_region_signals(const StencilSpec& spec, const FieldLayout& lay, int steps) {
  return dev::choose(spec, lay, steps).signals;
}

const char* hip_kernel_name(const StencilSpec& spec, const FieldLayout& lay, int steps) {
  return dev::kernel_name(dev::choose(spec, lay, steps).kernel);
}

// Generations rules (life_gen_bits, 3 .. 32 states in P = 2 .. 5 bit planes). 32768^2, density 0.5, GCells/s
// for K = 1 / 2 / 3 / 4 / 6 / 8, alternating in one process with life_rule_bits (HighLife: 2254 / 4461 /
// 6596 / 8679 / 12721 / 16262), best of 5 rounds of 100 sweeps, two runs within 0.5 % (profiles/r12_life_generations/):
//   C = 3  (P = 2)  2160 / 4238 / 6415 / 8577 / 12288 / 14581      C = 16 (P = 4)  2106 / 4288 / 6349 / 8022 / 9707 / 10257
//   C = 8  (P = 3)  2138 / 4213 / 6407 / 8478 / 11260 / 11794      C = 32 (P = 5)  2089 / 4212 / 5890 / 6948 / 8208 / 8983
// The deepest built sweep is the fastest per generation at every P; the naive kernel runs C = 3 at 394. More
// than 32 states have the naive single step only.
static int life_gen_depth(int states) { return states <= 32 ? 8 : 1; }
// per-sweep times against the same P's single step in that run: one pass over memory up to K = 6 / 4 / 4 / 2
// for P = 2 / 3 / 4 / 5, bound by the arithmetic (4 P + 3 ops per generation on top of life_rule_bits' 32) beyond
static double life_gen_cost(int states, int steps) {
  static const double c[4][9] = {{0.0, 1.0, 1.02, 1.01, 1.01, 0.0, 1.05, 0.0, 1.18},
                                 {0.0, 1.0, 1.02, 1.00, 1.01, 0.0, 1.14, 0.0, 1.45},
                                 {0.0, 1.0, 0.98, 1.00, 1.05, 0.0, 1.30, 0.0, 1.64},
                                 {0.0, 1.0, 0.99, 1.06, 1.20, 0.0, 1.53, 0.0, 1.86}};
  const int p = states <= 4 ? 0 : states <= 8 ? 1 : states <= 16 ? 2 : 3;
  if (states <= 32 && steps <= 8 && c[p][steps] > 0.0) return c[p][steps];
  return 1.0 + 0.05 * (steps - 1);
}

int hip_fused_depth(const StencilSpec& spec, int64_t nx) {
  switch (spec.kind) {
    case StencilKind::Jacobi5: return 8;
    case StencilKind::Box9:
      // the deepest sweep is the fastest per step for both dtypes: 16384^2 fp32 557 / 1166 / 1640 /
      // 2177 / 3462 / 3607 GCells/s for K = 1 / 2 / 3 / 4 / 6 / 8 (jacobi5 in the same call: 576 /
      // 1123 / 1706 / 2277 / 3400 / 4611), fp64 281 / 564 / 835 / 1104 / 1759 / 1901 (304 / 613 / 904 /
      // 1203 / 1639 / 2276); the sweeps stay at the memory roof up to K = 6 (profiles/r07_box9/)
      return 8;
    case StencilKind::Conv9:
      // 16384^2 fp32 542 / 1094 / 1552 / 2096 / 2554 / 2407 GCells/s for K = 1 / 2 / 3 / 4 / 6 / 8 (box9 in
      // the same call: 558 / 1166 / 1647 / 2177 / 3454 / 3607), fp64 276 / 551 / 905 / 1090 / 1556 / 1735
      // (280 / 565 / 836 / 1104 / 1761 / 1901): at the memory roof up to K = 4, bound by its arithmetic
      // (11 VALU ops per cell and level against box9's 7) from K = 6 on; fp32 K = 8 costs 1.8 single
      // steps per sweep and loses to K = 6 (profiles/r10_conv9/)
      return spec.dtype == DType::F64 ? 8 : 6;
    case StencilKind::Star7:
      // K = 3 is the fastest per step for both dtypes: 512^3 fp32 565 / 879 / 995 / 666 GCells/s for
      // K = 1 / 2 / 3 / 4 (heat7's kernels in the same call: 669 / 1300 / 1650 / 2031), fp64 294 / 473 /
      // 552 / 266 (322 / 618 / 731 / 1011). star7_tbk's strips are 4 / 4 / 3 (fp64 2) / 1 rows (deeper
      // strips spilled), so K = 4 updates 2.5 rows per row it stores (profiles/r09_star7/)
      return 3;
    case StencilKind::Star13:
      // 512^3 fp32 423 / 451 GCells/s for K = 1 / 2 (heat7's kernels in the same call: 670 / 1284, star7's
      // 563 / 882), fp64 270 / 217 (320 / 622, 294 / 471): the fp64 K = 2 sweep (strips of 3 rows, one wave
      // per SIMD) costs 2.49 single steps and loses; fp32 K = 2 wins by 6-7 % (profiles/r11_star13/)
      return spec.dtype == DType::F64 ? 1 : 2;
    case StencilKind::Life:
      // any other rule (life_rule_bits): 12 as well, by its own measurement. 32768^2, HighLife, GCells/s
      // for K = 1 / 2 / 3 / 4 / 6 / 8 / 12 / 16: 2232 / 4415 / 6532 / 8584 / 12656 / 16217 / 19233 / 16380
      // (Conway's kernels in the same call: 2438 / 4842 / 6329 / 8310 / 12157 / 16280 / 22639 / 22286);
      // K = 16 runs at 2 waves per SIMD (177-184 VGPRs) and loses (profiles/r08_life_rules/)
      if (spec.generations()) return life_gen_depth(spec.coef.states);
      return 12;
    case StencilKind::Box27:
      // K = 3 through box27_wxk for fp64 (512^3: 663 vs 527 GCells/s for box27_tbk K = 2), for fp32
      // rows of 1024 cells and more (1024^3: 1291 vs 1102, profiles/archive/r03_wxk/) and, since round 5's
      // whole-row blocks, for fp32 rows of 257..512 cells (512^3: 1332 vs 1092 for box27_tb2n K = 2,
      // profiles/r05_session_f/). MDFX_B27_WXK = 0 / 1 forces K = 2 / 3
      if (dev::knobs().b27_wxk == 1) return 3;
      if (dev::knobs().b27_wxk == 0) return 2;
      return (spec.dtype == DType::F64 || nx >= 1024 || (nx > 256 && nx <= 512)) ? 3 : 2;
    case StencilKind::Heat7:
      // K = 3 through heat7_wtk wherever its x segments cover at least 2/3 of the lane cells:
      // 1024^3 fp32 1617-1679 vs 1221-1232 GCells/s at K = 2 (round 2), 2048^3 fp32 1666 vs 1136,
      // 1024^3 fp64 823-825 vs 546, 2048^3 fp64 818 vs 556; since the natural-layout rows also
      // 512^3 fp32 (3 segments of 256 for 512 cells): 1311 vs 1230 (profiles/archive/r03_wtk/). K = 4
      // where heat7_wxk runs: its per-wave rows no longer grow with K, so the fourth step per pass
      // costs less than the HBM pass it saves (fp32; fp64 in round 4: 512^3 983 vs 740 GCells/s at
      // K = 3, 1024^3 1121 vs 885, 2048^3 + residual every 12 953 vs 890, profiles/r04_session_{o,p}/)
      // fp32 K = 5 (round 5): heat7_wxk in rows of 2 cells per lane (RowOps2f), whose half-size
      // rows leave room for the fifth level: 1024^3 2689 vs 2426 GCells/s at K = 4 in one process,
      // 1024^2 x 256 2639 vs 2399, x 128 2536 vs 2384, 768^3 2349 vs 1954, 512^3 2187 vs 2039,
      // 2048^2 x 512 2166 vs 2144 (profiles/r05_session_t/, r05_session_u/)
      // fp64 K = 5 (round 6): heat7_wxk in rows of 1 cell per lane (RowOps1d, the 2-cell fp32 rows'
      // register footprint; 54 of 64 lanes own a column), from rows of 2048 cells: 2048^3 + residual
      // every 20 1120 vs 1058 GCells/s at K = 4, while at 1024-cell rows its 19 x segments x 27 bands
      // (513 tiles on 256 CUs) lose to K = 4 (1011-1035 vs 1062-1080) (profiles/r06_session_b/)
      if (nx >= 512 && dev::heat7_wtk_xeff(nx, (int)dtype_size(spec.dtype), 3) >= 0.66) {
        if (spec.dtype == DType::F32 && dev::knobs().h7_wxk != 0) return 5;
        if (spec.dtype == DType::F64 && nx >= 2048 && dev::knobs().h7_wxk != 0) return 5;
        return dev::use_wxk(spec.dtype, nx, 4) ? 4 : 3;
      }
      return 2;
  }
  return 1;
}

// From the per-step rates of each fused depth on one MI355X (GCells/s; the time of a k-step sweep
// is k / rate_k): 3D 7-point fp32 1024^3 694 / 1300 / 1896 / 2350 for K = 1..4, fp64 347 / 546 /
// 885 / 1110 (profiles/archive/r03_wxk/first_ab.txt, r04_session_o/). Elsewhere a
// deeper sweep is taken to cost 5 % more per pass than a single step, which makes the plan the
// fewest sweeps with the deepest first.
double hip_sweep_cost(const StencilSpec& spec, int64_t nx, int steps) {
  if (steps <= 1) return 1.0;
  if (spec.kind == StencilKind::Heat7 && steps <= 5 && nx >= 1024) {
    // (fp32 K = 5 from the round-5 rates 1929 / 2399 / 2639 GCells/s for K = 3 / 4 / 5 at 1024^2 x
    // 256, scaled to the K = 4 entry; fp64 K = 5 from round 6's per-sweep times against K = 4: 2048^3
    // 38.4 vs 32.5 ms (x 1.18), 1024^3 x 1.31, profiles/r06_session_b/)
    // fp64 rows of 2048+ cells have their own row (round 6, per-sweep times at 2048^3: K = 3 28.8 ms
    // (heat7_wxk 3 + 1 rows, round 3's 897 GCells/s), K = 4 34.9, K = 5 38.4, against ~24.8 ms for a
    // single step; a residual every 12 steps then plans 5 + 4 + 3, which measured 1022 vs 961-985
    // GCells/s for depth 4's 4 + 4 + 4 on one box, profiles/r06_session_g/)
    static const double f32[6] = {0.0, 1.0, 1.07, 1.10, 1.18, 1.34};
    static const double f64[6] = {0.0, 1.0, 1.27, 1.18, 1.25, 1.64};
    static const double f64w[6] = {0.0, 1.0, 1.27, 1.16, 1.41, 1.55};
    if (spec.dtype == DType::F64) return (nx >= 2048 ? f64w : f64)[steps];
    return f32[steps];
  }
  if (spec.kind == StencilKind::Box9 && steps <= 8 && nx >= 8192) {
    // per-sweep times against a single step at 16384^2 (profiles/r07_box9/): a sweep of up to 6 steps
    // costs one pass over memory, K = 8 is bound by its arithmetic. (The default's 1.25 / 1.35 for
    // K = 6 / 8 cuts a 9-step residual interval into 8 + 1, 2.24 single-step times by these figures
    // against 1.99 for 6 + 3.)
    static const double f32[9] = {0.0, 1.0, 0.96, 1.02, 1.02, 0.0, 0.97, 0.0, 1.24};
    static const double f64[9] = {0.0, 1.0, 1.00, 1.01, 1.02, 0.0, 0.96, 0.0, 1.18};
    const double c = (spec.dtype == DType::F64 ? f64 : f32)[steps];
    if (c > 0.0) return c;
  }
  if (spec.kind == StencilKind::Conv9 && steps <= 8 && nx >= 8192) {
    // conv9_tbk's per-sweep times against its single step at 16384^2 (profiles/r10_conv9/): one pass over
    // memory up to K = 4, arithmetic-bound beyond (fp32 K = 8: more than K = 6 + 2)
    static const double f32[9] = {0.0, 1.0, 0.99, 1.05, 1.04, 0.0, 1.27, 0.0, 1.81};
    static const double f64[9] = {0.0, 1.0, 1.00, 0.92, 1.01, 0.0, 1.07, 0.0, 1.27};
    const double c = (spec.dtype == DType::F64 ? f64 : f32)[steps];
    if (c > 0.0) return c;
  }
  if (spec.kind == StencilKind::Star7 && steps <= 4) {
    // star7_tbk's per-sweep times against its single step at 512^3 (profiles/r09_star7/): the trapezoid's
    // redundant rows make every fused sweep cost more than one pass, and K = 4 more than two sweeps of 2
    static const double f32[5] = {0.0, 1.0, 1.29, 1.70, 3.39};
    static const double f64[5] = {0.0, 1.0, 1.24, 1.60, 4.41};
    return (spec.dtype == DType::F64 ? f64 : f32)[steps];
  }
  if (spec.kind == StencilKind::Star13 && steps == 2) {
    // star13_tbk's K = 2 sweep against its single step at 512^3, two repeats (profiles/r11_star13/): fp32
    // 0.2969-0.2981 ms per step against 0.3172-0.3176, fp64 0.6183-0.6190 against 0.4959-0.4965
    return spec.dtype == DType::F64 ? 2.49 : 1.87;
  }
  if (spec.kind == StencilKind::Life && spec.generations() && nx >= 8192) return life_gen_cost(spec.coef.states, steps);
  if (spec.kind == StencilKind::Life && !spec.conway() && steps <= 16 && nx >= 8192) {
    // life_rule_bits' per-sweep times against its own single step at 32768^2 (profiles/r08_life_rules/):
    // one pass over memory up to K = 8, bound by its arithmetic from K = 12 on, and K = 16 (2 waves per
    // SIMD) costs more than two sweeps of 8
    static const double c[17] = {0.0, 1.0, 1.01, 1.03, 1.04, 0.0, 1.06, 0.0, 1.10, 0.0, 0.0, 0.0, 1.39, 0.0, 0.0, 0.0, 2.18};
    if (c[steps] > 0.0) return c[steps];
  }
  return 1.0 + 0.05 * (steps - 1);
}

void hip_stencil(const StencilSpec& spec, const RegionArgs& a, void* stream) {
  const dev::Choice c = dev::choose(spec, a.lay, a.steps);
  if (a.lz2_end > a.lz2_begin) {
    // two regions in one call: heat7_wxk and box27_wxk sweep them in ONE launch (both boundary regions
    // of a slab: one fill of the device, one launch gap); every other kernel runs them one after the other
    if (!(c.pair && a.lz_end > a.lz_begin)) {
      RegionArgs r1 = a, r2 = a;
      r1.lz2_begin = r1.lz2_end = r2.lz2_begin = r2.lz2_end = 0;
      r2.lz_begin = a.lz2_begin;
      r2.lz_end = a.lz2_end;
      hip_stencil(spec, r1, stream);
      hip_stencil(spec, r2, stream);
      return;
    }
    MDFX_CHECK(a.lz2_begin >= a.lay.halo && a.lz2_end <= a.lay.halo + a.lay.nzl() && a.lz2_begin >= a.lz_end,
               "second region must lie inside the owned planes, after the first");
  }
  if (a.lz_end <= a.lz_begin) return;
  MDFX_CHECK(a.lz_begin >= a.lay.halo && a.lz_end <= a.lay.halo + a.lay.nzl(),
             "region must lie inside the owned planes");
  // (a slab that is the whole grid has no ghost planes to read: its faces are held)
  MDFX_CHECK(a.steps != 1 || stencil_radius(spec.kind) == 1 || a.lay.nzl() == a.lay.global.nz ||
                 a.lay.halo >= stencil_radius(spec.kind),
             format("a %s step on a slab reads %d ghost planes per side (halo %d)", stencil_name(spec.kind),
                    stencil_radius(spec.kind), a.lay.halo));
  dev::Geo g = dev::make_geo(a.lay, a.lz_begin, a.lz_end);
  g.lz2_begin = a.lz2_begin;
  g.lz2_end = a.lz2_end;
  g.min_rounds = std::max(1, std::min(4, a.min_rounds));
  if (a.sig) {
    MDFX_CHECK(c.signals && a.lz2_end <= a.lz2_begin && a.sig_z > a.lz_begin &&
                   a.sig_z <= a.lz_end,
               "a folded boundary (RegionArgs::sig) needs a one-region slab sweep through heat7_wxk");
    g.sig = a.sig;
    g.sig_z = a.sig_z;
    g.fold_release = dev::knobs().fold_release;
  }
  if (a.ly_end > a.ly_begin) {
    MDFX_CHECK(a.ly_begin >= a.lay.hy && a.ly_end <= a.lay.hy + a.lay.nyl(), "row range must lie inside the owned rows");
    g.ly_begin = a.ly_begin;
    g.ly_end = a.ly_end;
  }
  MDFX_CHECK(c.kernel != dev::Kernel::None,
             a.lay.pencil()
                 ? format("no fused %d-step kernel for %s %s on a pencil layout (heat7_wxk: the 3D 7-point, K = 3 / 4)",
                          a.steps, stencil_name(spec.kind), dtype_name(spec.dtype))
                 : format("no fused %d-step kernel for %s %s at nx=%lld (halo %d)", a.steps, stencil_name(spec.kind),
                          dtype_name(spec.dtype), (long long)a.lay.global.nx, a.lay.halo));
  hipStream_t s = (hipStream_t)stream;
  const StencilCoef& cf = spec.coef;
  const uint8_t* const u8in = (const uint8_t*)a.in;
  uint8_t* const u8out = (uint8_t*)a.out;
  // (T, tin, tout: the field type and the typed a.in / a.out)
#define MDFX_LAUNCH(...) MDFX_BY_DTYPE(spec.dtype, a.in, a.out, dev::__VA_ARGS__)
  switch (c.kernel) {
    case dev::Kernel::None: break;
    case dev::Kernel::Naive: dev::naive_launch(spec, g, a.in, a.out, a.resid, s); break;
    case dev::Kernel::Heat7Zw: MDFX_LAUNCH(launch_heat7<T>(g, tin, tout, (T)spec.rate(), a.resid, s)); break;
    case dev::Kernel::Heat7Tb2: MDFX_LAUNCH(launch_heat7_tb2<T>(g, tin, tout, (T)spec.rate(), a.resid, s)); break;
    case dev::Kernel::Heat7Tbk:
      MDFX_LAUNCH(launch_heat7_tbk<T>(g, tin, tout, (T)spec.rate(), a.steps, a.resid, s));
      break;
    case dev::Kernel::Heat7Wtk:
      dev::launch_heat7_wtk<double>(g, (const double*)a.in, (double*)a.out, spec.rate(), a.steps, a.resid, s);
      break;
    case dev::Kernel::Heat7Wxk:
      MDFX_LAUNCH(launch_heat7_wxk<T>(g, tin, tout, (T)spec.rate(), a.steps, a.resid, s));
      break;
    case dev::Kernel::Box27Zw: MDFX_LAUNCH(launch_box27<T>(g, tin, tout, cf, a.resid, s)); break;
    case dev::Kernel::Box27Tb2: MDFX_LAUNCH(launch_box27_tb2<T>(g, tin, tout, cf, a.resid, s)); break;
    case dev::Kernel::Box27Wxk: MDFX_LAUNCH(launch_box27_wxk<T>(g, tin, tout, cf, a.steps, a.resid, s)); break;
    case dev::Kernel::Jacobi5Wave:
      MDFX_LAUNCH(launch_jacobi5<T>(g, tin, tout, (T)spec.rate(), a.resid, s, spec.mixed_update()));
      break;
    case dev::Kernel::Jacobi5Tb2: MDFX_LAUNCH(launch_jacobi5_tb2<T>(g, tin, tout, (T)spec.rate(), a.resid, s)); break;
    case dev::Kernel::Jacobi5Tbk:
      MDFX_LAUNCH(launch_jacobi5_tbk<T>(g, tin, tout, (T)spec.rate(), a.steps, a.resid, s, spec.mixed_update()));
      break;
    case dev::Kernel::Box9: MDFX_LAUNCH(launch_box9<T>(g, tin, tout, cf, a.steps, a.resid, s)); break;
    case dev::Kernel::Conv9: MDFX_LAUNCH(launch_conv9<T>(g, tin, tout, cf, a.steps, a.resid, s)); break;
    case dev::Kernel::Star7: MDFX_LAUNCH(launch_star7<T>(g, tin, tout, cf, a.steps, a.resid, s)); break;
    case dev::Kernel::Star13: MDFX_LAUNCH(launch_star13<T>(g, tin, tout, cf, a.steps, a.resid, s)); break;
    case dev::Kernel::LifeWave: dev::launch_life(g, u8in, u8out, a.resid, s); break;
    case dev::Kernel::LifeTb2: dev::launch_life_tb2(g, u8in, u8out, a.resid, s); break;
    case dev::Kernel::LifeTbk: dev::launch_life_tbk(g, u8in, u8out, a.steps, a.resid, s); break;
    case dev::Kernel::LifeRule: dev::launch_life_rule(g, u8in, u8out, cf.birth, cf.survive, a.steps, a.resid, s); break;
    case dev::Kernel::LifeGen:
      dev::launch_life_gen(g, u8in, u8out, cf.birth, cf.survive, cf.states, a.steps, a.resid, s);
      break;
  }
#undef MDFX_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) MDFX_FAIL(std::string("stencil launch failed: ") + hipGetErrorString(e));
}

}  // namespace mdfx
