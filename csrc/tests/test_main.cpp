// Native unit tests (no framework dependency): slab math, layout, CPU oracle invariants,
// decomposition invariance through the engine on the CPU backend, GPU engine when a device exists.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "mdfx/solver.hpp"

using namespace mdfx;

static int g_fail = 0;
#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

static void test_slab() {
  for (int64_t nz : {7, 8, 1025, 33})
    for (int p : {1, 2, 3, 7}) {
      SlabDecomposition d(nz, p);
      EXPECT(d.z0(0) == 0 && d.z1(p - 1) == nz);
      for (int i = 0; i < p; ++i) {
        EXPECT(d.size(i) >= nz / p && d.size(i) <= nz / p + 1);
        for (int64_t z = d.z0(i); z < d.z1(i); ++z) EXPECT(d.owner(z) == i);
      }
    }
  bool threw = false;
  try {
    SlabDecomposition d(3, 4);
  } catch (const Error&) {
    threw = true;
  }
  EXPECT(threw);
}

static void test_layout() {
  FieldLayout l = FieldLayout::make(Extent3{100, 7, 20}, 5, 9, 1, DType::F32);
  EXPECT(l.pitch == 128 && l.plane == 128 * 7 && l.planes() == 6);
  EXPECT(l.lz(5) == 1 && l.gz(1) == 5);
  FieldLayout d = FieldLayout::make(Extent3{100, 1, 20}, 0, 20, 1, DType::F64);
  EXPECT(d.pitch * 8 % 256 == 0);
}

static void test_pencil_layout() {
  // 2 x 3 pencils of a 10 x 11 x 9 grid: ranks, neighbours, row ranges and the ghost-row layout
  PencilDecomposition d(Extent3{10, 11, 9}, 2, 3);
  EXPECT(d.pz() == 2 && d.py() == 3 && d.ranks() == 6);
  EXPECT(d.rz(4) == 1 && d.ry(4) == 1);
  EXPECT(d.neighbor(4, 0) == 1 && d.neighbor(4, 1) == -1 && d.neighbor(4, 2) == 3 && d.neighbor(4, 3) == 5);
  EXPECT(d.neighbor(0, 0) == -1 && d.neighbor(0, 2) == -1 && d.neighbor(5, 3) == -1);
  FieldLayout l = FieldLayout::make(Extent3{10, 11, 9}, d.z.z0(1), d.z.z1(1), 2, DType::F32, d.y.z0(1), d.y.z1(1), 2);
  EXPECT(l.pencil() && l.nyl() == d.y.size(1) && l.rows() == l.nyl() + 4 && l.plane == l.pitch * l.rows());
  EXPECT(l.owned_cells() == (int64_t)l.nzl() * l.nyl() * 10);
}

static std::vector<char> run_engine(StencilKind k, DType dt, Extent3 g, int P, int steps, bool gpu) {
  StencilSpec s;
  s.kind = k;
  s.dtype = dt;
  std::vector<int> ranks;
  std::vector<std::unique_ptr<Backend>> bes;
  for (int r = 0; r < P; ++r) {
    ranks.push_back(r);
    bes.push_back(gpu ? make_hip_backend(0) : make_cpu_backend());
  }
  Solver sol(s, g, P, ranks, std::move(bes), gpu ? make_loopback_transport() : make_host_transport());
  InitSpec is;
  is.kind = k == StencilKind::Life ? InitKind::LifeRandom : InitKind::Random;
  sol.init(is);
  sol.run(steps);
  std::vector<char> out;
  for (int i = 0; i < P; ++i) {
    const FieldLayout& l = sol.layout(i);
    std::vector<char> b((size_t)l.owned_cells() * l.esize());
    sol.read_owned(i, b.data());
    out.insert(out.end(), b.begin(), b.end());
  }
  return out;
}

// The dense global grid after `steps` steps of a pz x py pencil run (py = 1: slabs).
static std::vector<char> run_pencils(StencilKind k, DType dt, Extent3 g, int P, int py, int steps, int temporal,
                                     bool gpu) {
  StencilSpec s;
  s.kind = k;
  s.dtype = dt;
  std::vector<int> ranks;
  std::vector<std::unique_ptr<Backend>> bes;
  for (int r = 0; r < P; ++r) {
    ranks.push_back(r);
    bes.push_back(gpu ? make_hip_backend(0) : make_cpu_backend());
  }
  SolverOptions o;
  o.py = py;
  o.temporal = temporal;
  Solver sol(s, g, P, ranks, std::move(bes), gpu ? make_loopback_transport() : make_host_transport(), o);
  InitSpec is;
  is.kind = InitKind::Random;
  sol.init(is);
  sol.run(steps);
  const size_t es = dt == DType::F64 ? 8 : 4;
  std::vector<char> out((size_t)g.nx * g.ny * g.nz * es);
  for (int i = 0; i < P; ++i) {
    const FieldLayout& l = sol.layout(i);
    std::vector<char> b((size_t)l.owned_cells() * es);
    sol.read_owned(i, b.data());
    const size_t row = (size_t)g.nx * es;
    for (int64_t z = 0; z < l.nzl(); ++z)
      for (int64_t y = 0; y < l.nyl(); ++y)
        std::memcpy(&out[(((size_t)(l.z0 + z) * g.ny) + (size_t)(l.y0 + y)) * row],
                    &b[((size_t)z * l.nyl() + (size_t)y) * row], row);
  }
  return out;
}

static void test_pencil_invariance(bool gpu) {
  // pencils = one slab, bitwise: 7-point (single and fused steps) and 27-point (edge / corner ghosts)
  const Extent3 g{gpu ? 256 : 20, 18, 16};
  const auto h7 = run_pencils(StencilKind::Heat7, DType::F32, g, 1, 1, 7, 1, gpu);
  EXPECT(run_pencils(StencilKind::Heat7, DType::F32, g, 4, 2, 7, 1, gpu) == h7);
  EXPECT(run_pencils(StencilKind::Heat7, DType::F32, g, 6, 3, 7, gpu ? 3 : 2, gpu) == h7);
  const auto b27 = run_pencils(StencilKind::Box27, DType::F64, g, 1, 1, 5, 1, gpu);
  EXPECT(run_pencils(StencilKind::Box27, DType::F64, g, 4, 2, 5, 1, gpu) == b27);
}

static void test_invariance(bool gpu) {
  struct C {
    StencilKind k;
    DType d;
    Extent3 g;
  } cs[] = {{StencilKind::Heat7, DType::F32, {20, 9, 11}},
            {StencilKind::Box27, DType::F64, {13, 8, 9}},
            {StencilKind::Jacobi5, DType::F32, {30, 1, 17}},
            {StencilKind::Life, DType::U8, {40, 1, 21}}};
  for (auto& c : cs) {
    const auto base = run_engine(c.k, c.d, c.g, 1, 5, gpu);
    for (int p : {2, 3, 4}) EXPECT(run_engine(c.k, c.d, c.g, p, 5, gpu) == base);
    if (gpu) EXPECT(run_engine(c.k, c.d, c.g, 1, 5, false) == base);  // GPU == CPU oracle
  }
}

static void test_graph() {
  // eager vs hipGraph replay, loopback with 3 slabs on device 0
  int rtv = 0;
  (void)hipRuntimeGetVersion(&rtv);
  std::fprintf(stderr, "[graph probe] HIP runtime %d\n", rtv);
  for (int P : {1, 3}) {
    std::vector<std::vector<char>> outs;
    for (bool graph : {false, true}) {
      std::fprintf(stderr, "[graph probe] P=%d graph=%d: build\n", P, (int)graph);
      StencilSpec s;
      s.kind = StencilKind::Heat7;
      std::vector<int> ranks;
      std::vector<std::unique_ptr<Backend>> bes;
      for (int r = 0; r < P; ++r) {
        ranks.push_back(r);
        bes.push_back(make_hip_backend(0));
      }
      SolverOptions o;
      o.graph = graph;
      Solver sol(s, Extent3{64, 16, 20}, P, ranks, std::move(bes), make_loopback_transport(), o);
      InitSpec is;
      sol.init(is);
      std::fprintf(stderr, "[graph probe] run\n");
      sol.run(6);
      std::fprintf(stderr, "[graph probe] sync\n");
      sol.synchronize();
      std::vector<char> out;
      for (int i = 0; i < P; ++i) {
        const FieldLayout& l = sol.layout(i);
        std::vector<char> b((size_t)l.owned_cells() * l.esize());
        sol.read_owned(i, b.data());
        out.insert(out.end(), b.begin(), b.end());
      }
      outs.push_back(out);
      std::fprintf(stderr, "[graph probe] done\n");
    }
    EXPECT(outs[0] == outs[1]);
  }
}

// fused K-step sweeps (halo K) == single steps: every stencil at every fused depth its tuned kernels
// have (heat7_tbk / heat7_wtk / heat7_wxk up to K = 5, box27_wxk at K = 3, box9_tbk / conv9_tbk up to 8,
// star7_tbk up to 4, life_bits and, under a non-Conway rule, life_rule_bits up to 16), several slab
// counts, ragged and x-tiled (wider than one block) rows. Each run takes two full-depth sweeps and a
// tail, with a residual on the first; the devcheck build counts every one of these kernels'
// out-of-allocation accesses.
static void test_temporal(bool gpu) {
  struct C {
    StencilKind k;
    DType d;
    Extent3 g;
    std::vector<int> depths;
    const char* rule;
  } cs[] = {{StencilKind::Heat7, DType::F32, {1100, 9, 23}, {1, 2, 3, 4, 5}, nullptr},
            {StencilKind::Heat7, DType::F64, {77, 13, 19}, {1, 2, 3, 4, 5}, nullptr},
            {StencilKind::Box27, DType::F32, {300, 11, 17}, {1, 2, 3}, nullptr},
            {StencilKind::Jacobi5, DType::F64, {700, 1, 29}, {1, 2, 3}, nullptr},
            {StencilKind::Life, DType::U8, {2100, 1, 31}, {1, 2, 3}, nullptr},
            {StencilKind::Box9, DType::F32, {700, 1, 29}, {1, 2, 3, 4, 6, 8}, nullptr},
            {StencilKind::Conv9, DType::F64, {300, 1, 31}, {1, 2, 3, 4, 6, 8}, nullptr},
            {StencilKind::Star7, DType::F32, {130, 9, 17}, {1, 2, 3, 4}, nullptr},
            {StencilKind::Life, DType::U8, {2100, 1, 53}, {1, 2, 3, 4, 6, 8, 12, 16}, "B36/S23"}};
  for (auto& c : cs)
    for (int p : {1, 3}) {
      std::vector<std::vector<char>> outs;
      for (int t : c.depths) {
        StencilSpec s;
        s.kind = c.k;
        s.dtype = c.d;
        if (c.rule) life_rule_from_name(c.rule, s.coef.birth, s.coef.survive);
        std::vector<int> ranks;
        std::vector<std::unique_ptr<Backend>> bes;
        for (int r = 0; r < p; ++r) {
          ranks.push_back(r);
          bes.push_back(gpu ? make_hip_backend(0) : make_cpu_backend());
        }
        SolverOptions o;
        o.temporal = t;
        o.residual_every = std::max(4, t);
        Solver sol(s, c.g, p, ranks, std::move(bes), gpu ? make_loopback_transport() : make_host_transport(), o);
        InitSpec is;
        is.kind = c.k == StencilKind::Life ? InitKind::LifeRandom : InitKind::Random;
        sol.init(is);
        sol.run(std::max(9, 2 * c.depths.back() + 1));
        std::vector<char> out;
        for (int i = 0; i < p; ++i) {
          const FieldLayout& l = sol.layout(i);
          std::vector<char> b((size_t)l.owned_cells() * l.esize());
          sol.read_owned(i, b.data());
          out.insert(out.end(), b.begin(), b.end());
        }
        outs.push_back(out);
      }
      for (size_t i = 1; i < outs.size(); ++i) EXPECT(outs[0] == outs[i]);
    }
}

int main() {
  test_slab();
  test_layout();
  test_pencil_layout();
  test_invariance(false);
  test_pencil_invariance(false);
  test_temporal(false);
  if (hip_device_count() > 0) {
    test_invariance(true);
    test_pencil_invariance(true);
    test_temporal(true);
    test_graph();
#ifdef MDFX_DEVICE_CHECKS
    const int64_t v = hip_device_check_violations();
    std::printf("device checks: %lld out-of-allocation accesses\n", (long long)v);
    EXPECT(v == 0);
    // the checks themselves work: with the self-test's halved bound the same kernels count hits
    setenv("MDFX_DEVCHECK_SELFTEST", "1", 1);
    hip_reload_knobs();  // the knobs are cached
    (void)run_engine(StencilKind::Heat7, DType::F32, Extent3{64, 16, 20}, 2, 3, true);
    unsetenv("MDFX_DEVCHECK_SELFTEST");
    hip_reload_knobs();
    EXPECT(hip_device_check_violations() > v);
#endif
  }
  if (g_fail) {
    std::fprintf(stderr, "%d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("mdfx_tests: all passed%s\n", hip_device_count() > 0 ? " (cpu + gpu)" : " (cpu)");
  return 0;
}
