// Host entry points of the gfx950 stencil kernels, declared once: every file that defines one of
// them includes this header, and so do the dispatcher (init_dispatch.hip) and naive_launch
// (stencil_naive.hip), so a definition always sees the declaration its callers use.
#pragma once

#include "kcommon.hpp"
#include "mdfx/common.hpp"

// The one f32 / f64 switch: runs the statement with T = float or double by the field type DT, and
// with the untyped field pointers IN / OUT as `const T* tin` / `T* tout`.
#define MDFX_BY_DTYPE_ARM(TYPE, IN, OUT, ...) \
  {                                           \
    using T = TYPE;                           \
    const T* const tin = (const T*)(IN);      \
    T* const tout = (T*)(OUT);                \
    (void)tin, (void)tout;                    \
    __VA_ARGS__;                              \
  }
#define MDFX_BY_DTYPE(DT, IN, OUT, ...)                \
  do {                                                 \
    if ((DT) == DType::F32)                            \
      MDFX_BY_DTYPE_ARM(float, IN, OUT, __VA_ARGS__)   \
    else                                               \
      MDFX_BY_DTYPE_ARM(double, IN, OUT, __VA_ARGS__)  \
  } while (0)

namespace mdfx {
namespace dev {

// z-chunk of a one-pass sweep (stencil_heat.hip)
int pick_zc(int64_t planes, int64_t columns, int zc_max, int blocks_target);

// one cell per lane, every stencil family: the "naive" variant (stencil_naive.hip) ...
void naive_launch(const StencilSpec& spec, const Geo& g, const void* in, void* out, double* resid,
                  hipStream_t s);
// ... whose box9 / star7 / star13 kernels live in their families' files, for those files' build flags
template <class T>
void launch_box9_naive(const Geo& g, const T* in, T* out, const StencilCoef& c, double* resid, hipStream_t s);
template <class T>
void launch_star7_naive(const Geo& g, const T* in, T* out, const StencilCoef& c, double* resid, hipStream_t s);
template <class T>
void launch_star13_naive(const Geo& g, const T* in, T* out, const StencilCoef& c, double* resid, hipStream_t s);

// single steps: heat7_zw and jacobi5_wave (stencil_heat.hip), box27_zw (stencil_box27.hip)
template <class T>
void launch_heat7(const Geo& g, const T* in, T* out, T r, double* resid, hipStream_t s);
template <class T>
void launch_jacobi5(const Geo& g, const T* in, T* out, T r, double* resid, hipStream_t s, bool ref);
template <class T>
void launch_box27(const Geo& g, const T* in, T* out, const StencilCoef& c, double* resid,
                  hipStream_t s);

// 3D 7-point, 2 fused steps: heat7_tbk (rows within one block, stencil_heat_tbk.hip), heat7_tb2 x tiles
// (wider rows, stencil_heat_tb.hip)
template <class T>
void launch_heat7_tb2(const Geo& g, const T* in, T* out, T r, double* resid, hipStream_t s);
template <class T>
bool heat7_tb2_supported(const Geo& g);
template <class T>
void launch_heat7_tbk(const Geo& g, const T* in, T* out, T r, int steps, double* resid, hipStream_t s);
template <class T>
bool heat7_tbk_supported(const Geo& g, int steps);
// 3D 7-point, 3 / 4 fused steps in fp64: heat7_wtk (stencil_heat_wtk.hip)
template <class T>
void launch_heat7_wtk(const Geo& g, const T* in, T* out, T r, int steps, double* resid, hipStream_t s);
bool heat7_wtk_supported(int steps);
double heat7_wtk_xeff(int64_t nx, int esize, int steps);
// 3D 7-point, 3 / 4 / 5 fused steps, pencils too: heat7_wxk (stencil_heat_wxk.hip)
template <class T>
void launch_heat7_wxk(const Geo& g, const T* in, T* out, T r, int steps, double* resid, hipStream_t s);
bool heat7_wxk_supported(int steps);

// 2D 5-point: jacobi5_tb2 (2 steps), jacobi5_tbk (2, 3, 4, 6, 8 steps, and the mixed-precision
// update of ref_precision), stencil_heat_tb.hip
template <class T>
void launch_jacobi5_tb2(const Geo& g, const T* in, T* out, T r, double* resid, hipStream_t s);
template <class T>
void launch_jacobi5_tbk(const Geo& g, const T* in, T* out, T r, int steps, double* resid, hipStream_t s,
                        bool ref_precision);

// 3D 27-point: box27_tb2n (fp32) / box27_tbk (fp64) for 2 steps (stencil_box27.hip), box27_wxk for 3
// (stencil_box27_wxk.hip)
template <class T>
void launch_box27_tb2(const Geo& g, const T* in, T* out, const StencilCoef& c, double* resid, hipStream_t s);
template <class T>
bool box27_tb2_supported(const Geo& g);
template <class T>
void launch_box27_wxk(const Geo& g, const T* in, T* out, const StencilCoef& cf, int steps, double* resid,
                      hipStream_t s);

// 2D 9-point: box9_wave (steps = 1) and box9_tbk (2, 3, 4, 6, 8 fused steps), stencil_box9.hip
template <class T>
void launch_box9(const Geo& g, const T* in, T* out, const StencilCoef& c, int steps, double* resid, hipStream_t s);
// 2D 9-point with nine weights: conv9_tbk (1, 2, 3, 4, 6, 8 steps per sweep), stencil_conv9.hip
template <class T>
void launch_conv9(const Geo& g, const T* in, T* out, const StencilCoef& c, int steps, double* resid, hipStream_t s);
// 3D 7-point star with seven weights: star7_tbk (1, 2, 3, 4 steps per sweep), stencil_star7.hip
template <class T>
void launch_star7(const Geo& g, const T* in, T* out, const StencilCoef& c, int steps, double* resid, hipStream_t s);
// 3D radius-2 star: star13_tbk (1, 2 steps per sweep), stencil_star13.hip
template <class T>
void launch_star13(const Geo& g, const T* in, T* out, const StencilCoef& c, int steps, double* resid, hipStream_t s);

// Conway's rule: life_wave (1 generation), life_tb2 (2), life_bits (3, 4, 6, 8, 12, 16), stencil_life.hip
void launch_life(const Geo& g, const uint8_t* in, uint8_t* out, double* resid, hipStream_t s);
void launch_life_tb2(const Geo& g, const uint8_t* in, uint8_t* out, double* resid, hipStream_t s);
void launch_life_tbk(const Geo& g, const uint8_t* in, uint8_t* out, int steps, double* resid, hipStream_t s);
// any rule but Conway's: life_rule_bits (1, 2, 3, 4, 6, 8, 12, 16 generations), stencil_life_rule.hip
void launch_life_rule(const Geo& g, const uint8_t* in, uint8_t* out, uint32_t birth, uint32_t survive, int steps,
                      double* resid, hipStream_t s);
// a Generations rule with 3 .. 32 states: life_gen_bits (1, 2, 3, 4, 6, 8 generations), stencil_life_gen.hip
void launch_life_gen(const Geo& g, const uint8_t* in, uint8_t* out, uint32_t birth, uint32_t survive, int states,
                     int steps, double* resid, hipStream_t s);
bool life_gen_supported(int states, int steps);

}  // namespace dev
}  // namespace mdfx
