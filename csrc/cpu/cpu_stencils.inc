// CPU stencil kernels, included by cpu_kernels.cpp (baseline x86-64) and cpu_kernels_avx2.cpp
// (compiled with -mavx2 -mfma) inside a namespace named by MDFX_CPU_NS, so the two builds never
// share a symbol. Row-oriented: the Dirichlet edge columns are copied outside the inner loop,
// which is branch-free and vectorises; the point arithmetic is sm::* (exact fma), so every build
// is bitwise identical to the device kernels.
#ifndef MDFX_CPU_NS
#error "define MDFX_CPU_NS before including cpu_stencils.inc"
#endif

namespace mdfx {
namespace MDFX_CPU_NS {

// ny: storage rows per plane; gny / gy_off: the global row count and offset (global y = storage
// row + gy_off; a pencil layout keeps ghost rows); [yb, ye): the storage rows a region writes
struct Pl {
  int64_t pitch, plane, nx, ny, gnz, gz_off, gny, gy_off, yb, ye;
};

inline Pl pl_of(const FieldLayout& l) {
  return Pl{l.pitch, l.plane, l.global.nx, l.rows(), l.global.nz, l.z0 - l.halo, l.global.ny, l.y0 - l.hy,
            (int64_t)l.hy, (int64_t)l.hy + l.nyl()};
}

template <class T>
inline double row_resid(const T* o, const T* c, int64_t nx) {
  double acc = 0.0;
  for (int64_t x = 0; x < nx; ++x) {
    const double d = (double)o[x] - (double)c[x];
    acc += d * d;
  }
  return acc;
}

template <class T, bool RES>
void heat7_cpu(const T* in, T* out, const Pl& g, int64_t lb, int64_t le, T r, double* resid) {
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * (g.ye - g.yb) * g.nx > 262144)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    for (int64_t y = g.yb; y < g.ye; ++y) {
      const int64_t row = lz * g.plane + y * g.pitch;
      const T* __restrict__ c = in + row;
      T* __restrict__ o = out + row;
      const int64_t gy = y + g.gy_off;
      if (gz > 0 && gz < g.gnz - 1 && gy > 0 && gy < g.gny - 1 && g.nx > 2) {
        const T *__restrict__ ym = c - g.pitch, *__restrict__ yp = c + g.pitch;
        const T *__restrict__ zm = c - g.plane, *__restrict__ zp = c + g.plane;
        o[0] = c[0];
#pragma omp simd
        for (int64_t x = 1; x < g.nx - 1; ++x) o[x] = sm::heat7<T>(c[x], c[x - 1], c[x + 1], ym[x], yp[x], zm[x], zp[x], r);
        o[g.nx - 1] = c[g.nx - 1];
      } else {
        std::memcpy(o, c, (size_t)g.nx * sizeof(T));
      }
      if (RES) acc += row_resid(o, c, g.nx);
    }
  }
  if (RES) *resid += acc;
}

template <class T, bool RES>
void jacobi5_cpu(const T* in, T* out, const Pl& g, int64_t lb, int64_t le, T r, bool ref, double* resid) {
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * g.nx > 262144)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    const T* __restrict__ c = in + lz * g.plane;
    T* __restrict__ o = out + lz * g.plane;
    if (gz > 0 && gz < g.gnz - 1 && g.nx > 2) {
      const T *__restrict__ zm = c - g.plane, *__restrict__ zp = c + g.plane;
      o[0] = c[0];
      if (ref) {
        for (int64_t x = 1; x < g.nx - 1; ++x) o[x] = sm::jacobi5_ref<T>(c[x], c[x - 1], c[x + 1], zm[x], zp[x], r);
      } else {
#pragma omp simd
        for (int64_t x = 1; x < g.nx - 1; ++x) o[x] = sm::jacobi5<T>(c[x], c[x - 1], c[x + 1], zm[x], zp[x], r);
      }
      o[g.nx - 1] = c[g.nx - 1];
    } else {
      std::memcpy(o, c, (size_t)g.nx * sizeof(T));
    }
    if (RES) acc += row_resid(o, c, g.nx);
  }
  if (RES) *resid += acc;
}

template <class T, bool RES>
void box27_cpu(const T* in, T* out, const Pl& g, int64_t lb, int64_t le, const StencilCoef& cf, double* resid) {
  const T c0 = (T)cf.c0, c1 = (T)cf.c1, c2 = (T)cf.c2, c3 = (T)cf.c3;
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * (g.ye - g.yb) * g.nx > 131072)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    for (int64_t y = g.yb; y < g.ye; ++y) {
      const int64_t row = lz * g.plane + y * g.pitch;
      const T* __restrict__ c = in + row;
      T* __restrict__ o = out + row;
      const int64_t gy = y + g.gy_off;
      if (gz > 0 && gz < g.gnz - 1 && gy > 0 && gy < g.gny - 1 && g.nx > 2) {
        const int64_t P = g.pitch, Z = g.plane;
        o[0] = c[0];
#pragma omp simd
        for (int64_t x = 1; x < g.nx - 1; ++x) {
          // per-plane partials exactly as stencil_math.hpp / the device kernels
          T ce, cr, dg;
          const T* p = c + x - Z;
          ce = p[0];
          cr = (p[-1] + p[1]) + (p[-P] + p[P]);
          dg = (p[-P - 1] + p[-P + 1]) + (p[P - 1] + p[P + 1]);
          const T am = sm::box27_A<T>(ce, cr, dg, c1, c2, c3);
          p = c + x;
          ce = p[0];
          cr = (p[-1] + p[1]) + (p[-P] + p[P]);
          dg = (p[-P - 1] + p[-P + 1]) + (p[P - 1] + p[P + 1]);
          const T bc = sm::box27_B<T>(ce, cr, dg, c0, c1, c2);
          p = c + x + Z;
          ce = p[0];
          cr = (p[-1] + p[1]) + (p[-P] + p[P]);
          dg = (p[-P - 1] + p[-P + 1]) + (p[P - 1] + p[P + 1]);
          const T ap = sm::box27_A<T>(ce, cr, dg, c1, c2, c3);
          o[x] = sm::box27_combine<T>(am, bc, ap);
        }
        o[g.nx - 1] = c[g.nx - 1];
      } else {
        std::memcpy(o, c, (size_t)g.nx * sizeof(T));
      }
      if (RES) acc += row_resid(o, c, g.nx);
    }
  }
  if (RES) *resid += acc;
}

// 2D 9-point: per-row partials exactly as stencil_math.hpp / the device kernels
template <class T, bool RES>
void box9_cpu(const T* in, T* out, const Pl& g, int64_t lb, int64_t le, const StencilCoef& cf, double* resid) {
  const T c0 = (T)cf.c0, c1 = (T)cf.c1, c2 = (T)cf.c2;
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * g.nx > 262144)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    const T* __restrict__ c = in + lz * g.plane;
    T* __restrict__ o = out + lz * g.plane;
    if (gz > 0 && gz < g.gnz - 1 && g.nx > 2) {
      const T *__restrict__ zm = c - g.plane, *__restrict__ zp = c + g.plane;
      o[0] = c[0];
#pragma omp simd
      for (int64_t x = 1; x < g.nx - 1; ++x) {
        const T am = sm::box9_A<T>(zm[x], zm[x - 1] + zm[x + 1], c1, c2);
        const T bc = sm::box9_B<T>(c[x], c[x - 1] + c[x + 1], c0, c1);
        const T ap = sm::box9_A<T>(zp[x], zp[x - 1] + zp[x + 1], c1, c2);
        o[x] = sm::box9_combine<T>(am, bc, ap);
      }
      o[g.nx - 1] = c[g.nx - 1];
    } else {
      std::memcpy(o, c, (size_t)g.nx * sizeof(T));
    }
    if (RES) acc += row_resid(o, c, g.nx);
  }
  if (RES) *resid += acc;
}

// 2D 9-point with nine weights: sm::conv9, per-row partials exactly as the device kernels
template <class T, bool RES>
void conv9_cpu(const T* in, T* out, const Pl& g, int64_t lb, int64_t le, const StencilCoef& cf, double* resid) {
  T w[9];
  for (int i = 0; i < 9; ++i) w[i] = (T)cf.w9[i];
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * g.nx > 262144)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    const T* __restrict__ c = in + lz * g.plane;
    T* __restrict__ o = out + lz * g.plane;
    if (gz > 0 && gz < g.gnz - 1 && g.nx > 2) {
      const T *__restrict__ zm = c - g.plane, *__restrict__ zp = c + g.plane;
      o[0] = c[0];
#pragma omp simd
      for (int64_t x = 1; x < g.nx - 1; ++x) o[x] = sm::conv9<T>(zm + x, c + x, zp + x, w);
      o[g.nx - 1] = c[g.nx - 1];
    } else {
      std::memcpy(o, c, (size_t)g.nx * sizeof(T));
    }
    if (RES) acc += row_resid(o, c, g.nx);
  }
  if (RES) *resid += acc;
}

// 3D 7-point star with seven weights: sm::star7, the chain the device kernels evaluate
template <class T, bool RES>
void star7_cpu(const T* in, T* out, const Pl& g, int64_t lb, int64_t le, const StencilCoef& cf, double* resid) {
  const sm::Star7W<T> w{(T)cf.c0, (T)cf.wxm, (T)cf.wxp, (T)cf.wym, (T)cf.wyp, (T)cf.wzm, (T)cf.wzp};
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * (g.ye - g.yb) * g.nx > 262144)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    for (int64_t y = g.yb; y < g.ye; ++y) {
      const int64_t row = lz * g.plane + y * g.pitch;
      const T* __restrict__ c = in + row;
      T* __restrict__ o = out + row;
      const int64_t gy = y + g.gy_off;
      if (gz > 0 && gz < g.gnz - 1 && gy > 0 && gy < g.gny - 1 && g.nx > 2) {
        const T *__restrict__ ym = c - g.pitch, *__restrict__ yp = c + g.pitch;
        const T *__restrict__ zm = c - g.plane, *__restrict__ zp = c + g.plane;
        o[0] = c[0];
#pragma omp simd
        for (int64_t x = 1; x < g.nx - 1; ++x) o[x] = sm::star7<T>(c[x], c[x - 1], c[x + 1], ym[x], yp[x], zm[x], zp[x], w);
        o[g.nx - 1] = c[g.nx - 1];
      } else {
        std::memcpy(o, c, (size_t)g.nx * sizeof(T));
      }
      if (RES) acc += row_resid(o, c, g.nx);
    }
  }
  if (RES) *resid += acc;
}

// 3D radius-2 star: sm::star13, the chain the device kernels evaluate. A cell within 2 of a global face
// is copied through, so no row or plane pointer below leaves the grid.
template <class T, bool RES>
void star13_cpu(const T* in, T* out, const Pl& g, int64_t lb, int64_t le, const StencilCoef& cf, double* resid) {
  const sm::Star13W<T> w{(T)cf.c0, (T)cf.c1, (T)cf.c2};
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * (g.ye - g.yb) * g.nx > 262144)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    for (int64_t y = g.yb; y < g.ye; ++y) {
      const int64_t row = lz * g.plane + y * g.pitch;
      const T* __restrict__ c = in + row;
      T* __restrict__ o = out + row;
      const int64_t gy = y + g.gy_off;
      if (gz >= 2 && gz < g.gnz - 2 && gy >= 2 && gy < g.gny - 2 && g.nx > 4) {
        const T *__restrict__ ym1 = c - g.pitch, *__restrict__ yp1 = c + g.pitch;
        const T *__restrict__ ym2 = c - 2 * g.pitch, *__restrict__ yp2 = c + 2 * g.pitch;
        const T *__restrict__ zm1 = c - g.plane, *__restrict__ zp1 = c + g.plane;
        const T *__restrict__ zm2 = c - 2 * g.plane, *__restrict__ zp2 = c + 2 * g.plane;
        o[0] = c[0];
        o[1] = c[1];
#pragma omp simd
        for (int64_t x = 2; x < g.nx - 2; ++x)
          o[x] = sm::star13<T>(c[x], c[x - 1], c[x + 1], c[x - 2], c[x + 2], ym1[x], yp1[x], ym2[x], yp2[x], zm2[x],
                               zm1[x], zp1[x], zp2[x], w);
        o[g.nx - 2] = c[g.nx - 2];
        o[g.nx - 1] = c[g.nx - 1];
      } else {
        std::memcpy(o, c, (size_t)g.nx * sizeof(T));
      }
      if (RES) acc += row_resid(o, c, g.nx);
    }
  }
  if (RES) *resid += acc;
}

// CONWAY: sm::life_rule (B3/S23); otherwise sm::life_like with the spec's two masks
template <bool RES, bool CONWAY>
void life_cpu(const uint8_t* in, uint8_t* out, const Pl& g, int64_t lb, int64_t le, unsigned birth, unsigned survive,
              double* resid) {
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * g.nx > 1048576)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    const uint8_t* __restrict__ c = in + lz * g.plane;
    uint8_t* __restrict__ o = out + lz * g.plane;
    if (gz > 0 && gz < g.gnz - 1 && g.nx > 2) {
      const uint8_t *__restrict__ zm = c - g.plane, *__restrict__ zp = c + g.plane;
      o[0] = c[0];
#pragma omp simd
      for (int64_t x = 1; x < g.nx - 1; ++x) {
        const unsigned t = (unsigned)zm[x - 1] + zm[x] + zm[x + 1] + c[x - 1] + c[x] + c[x + 1] + zp[x - 1] +
                           zp[x] + zp[x + 1];
        o[x] = CONWAY ? sm::life_rule(t, c[x]) : sm::life_like(t, c[x], birth, survive);
      }
      o[g.nx - 1] = c[g.nx - 1];
    } else {
      std::memcpy(o, c, (size_t)g.nx);
    }
    if (RES) {
      int64_t n = 0;
      for (int64_t x = 0; x < g.nx; ++x) n += o[x] != c[x];
      acc += (double)n;
    }
  }
  if (RES) *resid += acc;
}

// a Generations rule (states > 2): only the cells in state 1 are counted, sm::life_gen decides
template <bool RES>
void life_gen_cpu(const uint8_t* in, uint8_t* out, const Pl& g, int64_t lb, int64_t le, unsigned birth,
                  unsigned survive, unsigned states, double* resid) {
  double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) if ((le - lb) * g.nx > 1048576)
  for (int64_t lz = lb; lz < le; ++lz) {
    const int64_t gz = lz + g.gz_off;
    const uint8_t* __restrict__ c = in + lz * g.plane;
    uint8_t* __restrict__ o = out + lz * g.plane;
    if (gz > 0 && gz < g.gnz - 1 && g.nx > 2) {
      const uint8_t *__restrict__ zm = c - g.plane, *__restrict__ zp = c + g.plane;
      o[0] = c[0];
      for (int64_t x = 1; x < g.nx - 1; ++x) {
        const unsigned n = (unsigned)(zm[x - 1] == 1) + (zm[x] == 1) + (zm[x + 1] == 1) + (c[x - 1] == 1) +
                           (c[x + 1] == 1) + (zp[x - 1] == 1) + (zp[x] == 1) + (zp[x + 1] == 1);
        o[x] = sm::life_gen(n, c[x], birth, survive, states);
      }
      o[g.nx - 1] = c[g.nx - 1];
    } else {
      std::memcpy(o, c, (size_t)g.nx);
    }
    if (RES) {
      int64_t n = 0;
      for (int64_t x = 0; x < g.nx; ++x) n += o[x] != c[x];
      acc += (double)n;
    }
  }
  if (RES) *resid += acc;
}

template <bool RES>
void region_t(const StencilSpec& spec, const RegionArgs& a) {
  Pl g = pl_of(a.lay);
  if (a.ly_end > a.ly_begin) {  // a row range (pencil boundary strips; widened fused steps)
    g.yb = a.ly_begin;
    g.ye = a.ly_end;
  }
  switch (spec.kind) {
    case StencilKind::Heat7:
      if (spec.dtype == DType::F32)
        heat7_cpu<float, RES>((const float*)a.in, (float*)a.out, g, a.lz_begin, a.lz_end, (float)spec.rate(), a.resid);
      else
        heat7_cpu<double, RES>((const double*)a.in, (double*)a.out, g, a.lz_begin, a.lz_end, spec.rate(), a.resid);
      break;
    case StencilKind::Jacobi5:
      if (spec.dtype == DType::F32)
        jacobi5_cpu<float, RES>((const float*)a.in, (float*)a.out, g, a.lz_begin, a.lz_end, (float)spec.rate(),
                                spec.coef.ref_precision, a.resid);
      else
        jacobi5_cpu<double, RES>((const double*)a.in, (double*)a.out, g, a.lz_begin, a.lz_end, spec.rate(),
                                 spec.coef.ref_precision, a.resid);
      break;
    case StencilKind::Box27:
      if (spec.dtype == DType::F32)
        box27_cpu<float, RES>((const float*)a.in, (float*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      else
        box27_cpu<double, RES>((const double*)a.in, (double*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      break;
    case StencilKind::Box9:
      if (spec.dtype == DType::F32)
        box9_cpu<float, RES>((const float*)a.in, (float*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      else
        box9_cpu<double, RES>((const double*)a.in, (double*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      break;
    case StencilKind::Star7:
      if (spec.dtype == DType::F32)
        star7_cpu<float, RES>((const float*)a.in, (float*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      else
        star7_cpu<double, RES>((const double*)a.in, (double*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      break;
    case StencilKind::Conv9:
      if (spec.dtype == DType::F32)
        conv9_cpu<float, RES>((const float*)a.in, (float*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      else
        conv9_cpu<double, RES>((const double*)a.in, (double*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      break;
    case StencilKind::Star13:
      if (spec.dtype == DType::F32)
        star13_cpu<float, RES>((const float*)a.in, (float*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      else
        star13_cpu<double, RES>((const double*)a.in, (double*)a.out, g, a.lz_begin, a.lz_end, spec.coef, a.resid);
      break;
    case StencilKind::Life:
      if (spec.generations())
        life_gen_cpu<RES>((const uint8_t*)a.in, (uint8_t*)a.out, g, a.lz_begin, a.lz_end, spec.coef.birth,
                          spec.coef.survive, (unsigned)spec.coef.states, a.resid);
      else if (spec.conway())
        life_cpu<RES, true>((const uint8_t*)a.in, (uint8_t*)a.out, g, a.lz_begin, a.lz_end, 0, 0, a.resid);
      else
        life_cpu<RES, false>((const uint8_t*)a.in, (uint8_t*)a.out, g, a.lz_begin, a.lz_end, spec.coef.birth,
                             spec.coef.survive, a.resid);
      break;
  }
}

void region(const StencilSpec& spec, const RegionArgs& a) {
  if (a.resid)
    region_t<true>(spec, a);
  else
    region_t<false>(spec, a);
}

}  // namespace MDFX_CPU_NS
}  // namespace mdfx
