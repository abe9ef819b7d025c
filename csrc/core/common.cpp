// mdfx core: error helpers, enum names, layout and slab decomposition math.
#include <algorithm>
#include <csignal>
#include <cstdarg>
#include <cstdlib>
#include <execinfo.h>
#include <unistd.h>
#include <cstdio>
#include <string>

#include "mdfx/common.hpp"
#include "mdfx/grid.hpp"

namespace mdfx {

namespace {
// MDFX_SEGV_BACKTRACE=1: print the native stack on a crash (host-side debugging on the GPU box,
// where debuggers are not available).
void segv_handler(int sig) {
  void* frames[64];
  const int n = backtrace(frames, 64);
  const char msg[] = "\n[mdfx] fatal signal, native backtrace:\n";
  (void)!write(2, msg, sizeof(msg) - 1);
  backtrace_symbols_fd(frames, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
struct SegvInstaller {
  SegvInstaller() {
    const char* v = std::getenv("MDFX_SEGV_BACKTRACE");
    if (v && *v == '1') {
      void* warm[4];
      (void)backtrace(warm, 4);  // load the unwinder now, not inside the handler
      struct sigaction sa {};
      sa.sa_handler = segv_handler;
      sa.sa_flags = SA_RESETHAND | SA_NODEFER;
      sigaction(SIGSEGV, &sa, nullptr);
      sigaction(SIGABRT, &sa, nullptr);
    }
  }
} g_segv_installer;
}  // namespace

void throw_error(const char* file, int line, const std::string& msg) {
  const char* base = file;
  for (const char* p = file; *p; ++p)
    if (*p == '/') base = p + 1;
  throw Error(std::string("[mdfx ") + base + ":" + std::to_string(line) + "] " + msg);
}

std::string format(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return std::string(buf);
}

const char* dtype_name(DType t) {
  switch (t) {
    case DType::F32: return "f32";
    case DType::F64: return "f64";
    case DType::U8: return "u8";
  }
  return "?";
}

DType dtype_from_name(const std::string& s) {
  if (s == "f32" || s == "float32" || s == "float") return DType::F32;
  if (s == "f64" || s == "float64" || s == "double") return DType::F64;
  if (s == "u8" || s == "uint8") return DType::U8;
  MDFX_FAIL("unknown dtype '" + s + "' (f32|f64|u8)");
}

const char* stencil_name(StencilKind k) {
  switch (k) {
    case StencilKind::Jacobi5: return "jacobi5";
    case StencilKind::Life: return "life";
    case StencilKind::Heat7: return "heat7";
    case StencilKind::Box27: return "box27";
    case StencilKind::Box9: return "box9";
    case StencilKind::Star7: return "star7";
    case StencilKind::Star13: return "star13";
    case StencilKind::Conv9: return "conv9";
  }
  return "?";
}

StencilKind stencil_from_name(const std::string& s) {
  if (s == "jacobi5" || s == "5" || s == "mdf" || s == "5pt") return StencilKind::Jacobi5;
  if (s == "life" || s == "gol") return StencilKind::Life;
  if (s == "heat7" || s == "7" || s == "jacobi7" || s == "7pt") return StencilKind::Heat7;
  if (s == "box27" || s == "27" || s == "27pt") return StencilKind::Box27;
  if (s == "box9" || s == "9" || s == "9pt") return StencilKind::Box9;
  if (s == "star7" || s == "s7") return StencilKind::Star7;
  if (s == "star13" || s == "13" || s == "s13") return StencilKind::Star13;
  if (s == "conv9" || s == "c9" || s == "3x3") return StencilKind::Conv9;
  MDFX_FAIL("unknown stencil '" + s + "' (5|7|9|27|star7|star13|conv9|life)");
}

void life_rule_from_name(const std::string& s, StencilCoef& coef) {
  const auto bad = [&]() {
    MDFX_FAIL("bad Life rule '" + s + "' (B<digits 0-8>/S<digits 0-8>[/C<states 2-256>], e.g. B36/S23, B2/S345/C4)");
  };
  uint32_t m[2] = {0, 0};
  size_t i = 0;
  for (int side = 0; side < 2; ++side) {
    if (i >= s.size() || (s[i] | 0x20) != (side == 0 ? 'b' : 's')) bad();
    for (++i; i < s.size() && s[i] >= '0' && s[i] <= '8'; ++i) m[side] |= 1u << (s[i] - '0');
    if (side == 0) {
      if (i >= s.size() || s[i] != '/') bad();
      ++i;
    }
  }
  int states = 2;
  if (i < s.size()) {  // "/C<n>"
    if (s[i] != '/' || i + 1 >= s.size() || (s[i + 1] | 0x20) != 'c') bad();
    const size_t first = i + 2;
    states = 0;
    for (i = first; i < s.size() && s[i] >= '0' && s[i] <= '9' && i < first + 3; ++i) states = states * 10 + (s[i] - '0');
    if (i == first || i != s.size() || states < 2 || states > 256) bad();
  }
  coef.birth = m[0];
  coef.survive = m[1];
  coef.states = states;
}

void life_rule_from_name(const std::string& s, uint32_t& birth, uint32_t& survive) {
  StencilCoef c;
  life_rule_from_name(s, c);
  if (c.states > 2) MDFX_FAIL("bad Life rule '" + s + "': a rule of two masks has two states, not " + std::to_string(c.states));
  birth = c.birth;
  survive = c.survive;
}

std::string life_rule_name(uint32_t birth, uint32_t survive, int states) {
  std::string s = "B";
  for (int n = 0; n <= 8; ++n)
    if (birth >> n & 1u) s += (char)('0' + n);
  s += "/S";
  for (int n = 0; n <= 8; ++n)
    if (survive >> n & 1u) s += (char)('0' + n);
  if (states > 2) s += "/C" + std::to_string(states);
  return s;
}

void star7_check_weights(const StencilCoef& c) {
  const double w[7] = {c.c0, c.wxm, c.wxp, c.wym, c.wyp, c.wzm, c.wzp};
  for (double v : w)
    if (!std::isfinite(v)) MDFX_FAIL("star7 weights must be finite (c0, xm, xp, ym, yp, zm, zp)");
}

// exactly `count` comma-separated finite numbers into w; false for anything else
static bool weights_from_text(const std::string& s, double* w, int count) {
  int n = 0;
  size_t pos = 0;
  bool ok = !s.empty();
  while (ok && pos <= s.size()) {
    const size_t end = std::min(s.find(',', pos), s.size());
    const std::string part = s.substr(pos, end - pos);
    char* tail = nullptr;
    const double v = std::strtod(part.c_str(), &tail);
    ok = !part.empty() && tail && *tail == '\0' && std::isfinite(v) && n < count;
    if (ok) w[n++] = v;
    pos = end + 1;
  }
  return ok && n == count;
}

void star13_check_weights(const StencilCoef& c) {
  if (!std::isfinite(c.c0) || !std::isfinite(c.c1) || !std::isfinite(c.c2))
    MDFX_FAIL("star13 weights must be finite (c0, c1, c2)");
}

void star7_weights_from_text(const std::string& s, StencilCoef& coef) {
  double w[7];
  if (!weights_from_text(s, w, 7))
    MDFX_FAIL("star7 weights '" + s + "': expected seven comma-separated finite numbers c0,xm,xp,ym,yp,zm,zp");
  coef.c0 = w[0];
  coef.wxm = w[1];
  coef.wxp = w[2];
  coef.wym = w[3];
  coef.wyp = w[4];
  coef.wzm = w[5];
  coef.wzp = w[6];
}

void conv9_check_weights(const StencilCoef& c) {
  for (double v : c.w9)
    if (!std::isfinite(v)) MDFX_FAIL("conv9 weights must be finite (nine, row-major)");
}

void conv9_weights_from_text(const std::string& s, StencilCoef& coef) {
  double w[9];
  if (!weights_from_text(s, w, 9))
    MDFX_FAIL("conv9 weights '" + s + "': expected nine comma-separated finite numbers, row-major (nw,n,ne,w,c,e,sw,s,se)");
  std::copy(w, w + 9, coef.w9);
}

FieldLayout FieldLayout::make(Extent3 g, int64_t z0, int64_t z1, int halo, DType dt, int64_t y0, int64_t y1, int hy) {
  MDFX_CHECK(g.nx >= 1 && g.ny >= 1 && g.nz >= 1, "grid extents must be positive");
  MDFX_CHECK(0 <= z0 && z0 <= z1 && z1 <= g.nz, "owned plane range out of the grid");
  MDFX_CHECK(halo >= 1, "halo must be >= 1");
  if (y1 < 0) y1 = g.ny;
  MDFX_CHECK(0 <= y0 && y0 < y1 && y1 <= g.ny, "owned row range out of the grid");
  MDFX_CHECK(hy >= 0 && (hy == 0 || g.ny > 1), "ghost rows need a 3D grid");
  FieldLayout l;
  l.global = g;
  l.z0 = z0;
  l.z1 = z1;
  l.halo = halo;
  l.y0 = y0;
  l.y1 = y1;
  l.hy = hy;
  l.dtype = dt;
  const int64_t align = kRowAlignBytes / (int64_t)dtype_size(dt);
  l.pitch = (g.nx + align - 1) / align * align;
  l.plane = l.pitch * l.rows();
  return l;
}

SlabDecomposition::SlabDecomposition(int64_t nz_, int parts_) : nz(nz_), parts(parts_) {
  MDFX_CHECK(parts >= 1, "need at least one part");
  MDFX_CHECK(nz >= parts, format("cannot split %lld planes over %d ranks", (long long)nz, parts));
}

int64_t SlabDecomposition::z0(int p) const {
  // first (nz % parts) parts get one extra plane
  const int64_t base = nz / parts, rem = nz % parts;
  return (int64_t)p * base + std::min<int64_t>(p, rem);
}

int SlabDecomposition::owner(int64_t gz) const {
  MDFX_CHECK(gz >= 0 && gz < nz, "plane outside the grid");
  const int64_t base = nz / parts, rem = nz % parts;
  const int64_t split = rem * (base + 1);
  if (gz < split) return (int)(gz / (base + 1));
  return (int)(rem + (gz - split) / base);
}

}  // namespace mdfx
