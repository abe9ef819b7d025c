// mdfx — MI355X-native multi-GPU finite-difference stencil engine.
// Common types, enums and error handling shared by every layer.
//
// Reference parity: the reference (Rodrigovicente/MPI-CUDA-Process) checks no return codes at all
// (SURVEY.md §0.3 D18); every HIP / RCCL / system call here goes through MDFX_* checks that throw
// mdfx::Error carrying file:line, so a failing rank fails loudly instead of hanging (D4).
#pragma once

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <cmath>
#include <string>

namespace mdfx {

class Error : public std::runtime_error {
 public:
  explicit Error(const std::string& m) : std::runtime_error(m) {}
};

[[noreturn]] void throw_error(const char* file, int line, const std::string& msg);

#define MDFX_CHECK(cond, msg)                                                      \
  do {                                                                             \
    if (!(cond)) ::mdfx::throw_error(__FILE__, __LINE__, std::string("check failed: ") + #cond + " — " + (msg)); \
  } while (0)

#define MDFX_FAIL(msg) ::mdfx::throw_error(__FILE__, __LINE__, (msg))

// Element types of a field. U8 is the Game-of-Life cell type (the reference used int, 4x the
// bytes for a 1-bit state: kernel.cu:10).
enum class DType : int { F32 = 0, F64 = 1, U8 = 2 };

inline size_t dtype_size(DType t) {
  switch (t) {
    case DType::F32: return 4;
    case DType::F64: return 8;
    case DType::U8: return 1;
  }
  return 0;
}
const char* dtype_name(DType t);
DType dtype_from_name(const std::string& s);

// Stencil families. 2D kinds store an h x w grid as (nx = w, ny = 1, nz = h): rows are the
// split ("plane") axis, exactly like the reference's row-slab split (MDF_kernel.cu:30,54).
enum class StencilKind : int {
  Jacobi5 = 0,  // 2D 5-point heat / Jacobi (reference MDF update, MDF_kernel.cu:20)
  Life = 1,     // 2D Moore-8 B3/S23 Game of Life (reference kernel.cu:66)
  Heat7 = 2,    // 3D 7-point heat / Jacobi (BASELINE.json configs 2, 3, 5)
  Box27 = 3,    // 3D 27-point weighted stencil (BASELINE.json config 4)
  Box9 = 4,     // 2D 9-point weighted stencil (centre, edge and corner weights)
  Star7 = 5,    // 3D 7-point star with seven independent weights (anisotropy, advection, decay)
  Conv9 = 6,    // 2D 9-point stencil with nine independent weights (any 3x3 linear update)
  Star13 = 7,   // 3D radius-2 star: the 13 points of the fourth-order Laplacian (centre, 6 at 1, 6 at 2)
};
const char* stencil_name(StencilKind k);
StencilKind stencil_from_name(const std::string& s);
inline bool stencil_is_2d(StencilKind k) {
  return k == StencilKind::Jacobi5 || k == StencilKind::Life || k == StencilKind::Box9 || k == StencilKind::Conv9;
}
// How far the stencil reaches along each axis. One fused step consumes `radius` ghost planes per side,
// and the held (Dirichlet) frame is `radius` cells thick: a cell is copied through iff one of its
// coordinates is within `radius` of a global face, so no update reads outside the grid.
inline int stencil_radius(StencilKind k) { return k == StencilKind::Star13 ? 2 : 1; }

// Coefficients. Jacobi5/Heat7: u' = u + r * (sum_neighbours - 2d * u). Box27:
// u' = c0*u + c1*sum(6 faces) + c2*sum(12 edges) + c3*sum(8 corners). Box9:
// u' = c0*u + c1*sum(4 edges) + c2*sum(4 corners) (c3 unused). Star7:
// u' = c0*u + wxm*u(x-1) + wxp*u(x+1) + wym*u(y-1) + wyp*u(y+1) + wzm*u(z-1) + wzp*u(z+1), evaluated as
// sm::star7; its default c0 is kStar7C0 (c0 is shared with the box families, whose default is 0.25).
// Sum |w| <= 1 keeps the max-norm from growing. Conv9: u' = sum over dz, dx in {-1, 0, 1} of
// w9[3*(dz+1) + (dx+1)] * u(z+dz, x+dx) (row-major; z is the row axis, x runs along the row), evaluated as
// sm::conv9. Its default is a diffusion with a positive cross term, weights non-negative and summing to 1.
// Star13: u' = c0*u + c1*sum(the 6 neighbours at distance 1) + c2*sum(the 6 at distance 2 along the axes),
// evaluated as sm::star13 (c3 unused). Its defaults kStar13C0/C1/C2 are the explicit fourth-order heat step
// u + r * Lap4(u) with r = 0.1: c0 = 1 - 7.5 r, c1 = 4 r / 3, c2 = -r / 12; they sum to 1, sum |w| = 1.1.
constexpr double kStar7C0 = 0.30;
constexpr double kStar13C0 = 0.25, kStar13C1 = 2.0 / 15.0, kStar13C2 = -1.0 / 120.0;
struct StencilCoef {
  double r = -1.0;  // < 0 -> default 1/(2d) (Jacobi)
  double c0 = 0.25, c1 = 1.0 / 20.0, c2 = 1.0 / 40.0, c3 = 3.0 / 160.0;
  double wxm = 0.20, wxp = 0.20, wym = 0.10, wyp = 0.10, wzm = 0.05, wzp = 0.05;  // Star7 neighbour weights
  double w9[9] = {0.06, 0.10, 0.02, 0.14, 0.36, 0.14, 0.02, 0.10, 0.06};  // Conv9 weights, row-major
  // 2D MDF only: evaluate the update exactly as the reference does (sm::jacobi5_ref: fp32 sum and
  // -4u, fp64 scale and add, one more rounding at the store) instead of wholly in the field type.
  // See StencilSpec::mixed_update() for when the two can differ at all.
  bool ref_precision = false;
  // Life only: the outer-totalistic Moore rule as two 9-bit masks. Bit n of `birth` set: a dead cell
  // with n live neighbours becomes alive; bit n of `survive` set: a live cell with n live neighbours
  // stays alive. The default is Conway's B3/S23.
  uint32_t birth = 0x008, survive = 0x00C;
  // Life only: the number of cell states C of a Generations rule (B/S/C), 2 .. 256. State 0 is dead, 1
  // alive, 2 .. C-1 dying; only state 1 counts as a neighbour. A live cell that does not survive
  // becomes 2 % C, a dying cell (s + 1) % C. 2 is a plain Life-like rule.
  int states = 2;
};

// A Life-like rule in B/S notation: "B36/S23", case-insensitive, digits 0..8 in any order, either
// side may be empty ("B2/S"); optionally a Generations rule "B2/S345/C4" with a decimal state count
// 2 .. 256. Anything else throws an Error that names the text. The two-mask form takes two-state
// rules only ("/C2" included) and throws on more states.
void life_rule_from_name(const std::string& s, StencilCoef& coef);
void life_rule_from_name(const std::string& s, uint32_t& birth, uint32_t& survive);
// canonical form, digits ascending; "/C<states>" appended when states > 2
std::string life_rule_name(uint32_t birth, uint32_t survive, int states = 2);

// Star7 weights as text: "c0,xm,xp,ym,yp,zm,zp", seven comma-separated finite numbers. Any other count,
// a non-number or a non-finite value throws an Error that names the text.
void star7_weights_from_text(const std::string& s, StencilCoef& coef);
void star7_check_weights(const StencilCoef& coef);  // every Star7 weight finite, else an Error

// Conv9 weights as text: nine comma-separated finite numbers, row-major (the row above first, west to
// east). Any other count, a non-number or a non-finite value throws an Error that names the text.
void conv9_weights_from_text(const std::string& s, StencilCoef& coef);
void conv9_check_weights(const StencilCoef& coef);  // every Conv9 weight finite, else an Error
void star13_check_weights(const StencilCoef& coef);  // c0, c1, c2 finite, else an Error

struct StencilSpec {
  StencilKind kind = StencilKind::Heat7;
  DType dtype = DType::F32;
  StencilCoef coef;
  // Conway's rule runs the B3/S23 kernels (life_wave, life_tb2, life_bits, sm::life_rule); every
  // other two-state rule runs the table-driven ones (life_rule_bits, sm::life_like), and a rule
  // with more states the Generations ones (life_gen_bits, sm::life_gen)
  bool conway() const { return coef.birth == 0x008u && coef.survive == 0x00Cu && coef.states == 2; }
  bool generations() const { return coef.states > 2; }
  double rate() const {  // effective r for 5/7-pt
    if (coef.r >= 0) return coef.r;
    return kind == StencilKind::Jacobi5 ? 0.25 : 1.0 / 6.0;
  }
  // Whether ref_precision can change a single bit of the result. The reference evaluates
  // round_f32(round_f64(r*t + u)) with t = fma_f32(-4, u, s); the field-type update is fma_f32(r, t, u)
  // = round_f32(r*t + u), one rounding of the exact value. When r is a power of two, r*t is exact
  // with 24 significant bits, so r*t + u is exact in fp64 unless the two exponents are more than 28
  // apart; then the smaller term is under 2^-28 of the larger, both the exact and the fp64-rounded
  // sum lie strictly inside the larger term's half-ulp interval, and both round to it. So with a
  // power-of-two r (the reference's 0.25) the two evaluations are bitwise identical for every input
  // (subnormals included: fp64 holds every fp32 subnormal product exactly), and the fused field-type
  // kernels serve ref_precision. An fp64 field evaluates the reference's update in one fp64 fma
  // either way. Only fp32 with another r needs the mixed kernels (tests/test_cpu_engine.py).
  bool mixed_update() const {
    if (!coef.ref_precision || kind != StencilKind::Jacobi5 || dtype != DType::F32) return false;
    int e = 0;
    const float r = (float)rate();
    return !(r > 0.0f && std::frexp(r, &e) == 0.5f);
  }
};

struct Extent3 {
  int64_t nx = 1, ny = 1, nz = 1;
  int64_t cells() const { return nx * ny * nz; }
};

// Where a field lives. CPU is the reference/oracle backend; HIP is the gfx950 device path.
enum class DeviceKind : int { CPU = 0, HIP = 1 };

std::string format(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

}  // namespace mdfx
