// Canonical point-update arithmetic, shared verbatim by the gfx950 kernels and the CPU oracle so
// that results are bitwise reproducible across backends, kernel variants and decompositions.
//
// Reference parity:
//   MDF update  MDF_kernel.cu:20  new = 0.25*(E+W+N+S - 4u) + u, evaluated there with an fp32 sum
//               and an fp64 scale/add. Here the whole update stays in the field's
//               dtype: s = ((W+E)+N)+S; u' = fma(r, fma(-4, u, s), u).
//   GoL rule    kernel.cu:66   alive' = n==3 || (n==2 && alive). With T = 3x3 sum including self
//               this is T==3 || (T==4 && alive).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define MDFX_HDI __host__ __device__ __forceinline__
#else
#define MDFX_HDI inline
#endif

namespace mdfx {
namespace sm {

MDFX_HDI float fmaT(float a, float b, float c) { return fmaf(a, b, c); }
MDFX_HDI double fmaT(double a, double b, double c) { return fma(a, b, c); }

// 3D 7-point heat / Jacobi: s = ((((xm+xp)+ym)+yp)+zm)+zp ; u' = u + r*(s - 6u)
template <class T>
MDFX_HDI T heat7(T c, T xm, T xp, T ym, T yp, T zm, T zp, T r) {
  const T s = ((((xm + xp) + ym) + yp) + zm) + zp;
  return fmaT(r, fmaT(T(-6), c, s), c);
}

// 2D 5-point (rows are the z axis): s = ((xm+xp)+zm)+zp ; u' = u + r*(s - 4u)
template <class T>
MDFX_HDI T jacobi5(T c, T xm, T xp, T zm, T zp, T r) {
  const T s = ((xm + xp) + zm) + zp;
  return fmaT(r, fmaT(T(-4), c, s), c);
}

// The reference's own evaluation of the MDF update (MDF_kernel.cu:20), for pinning its
// semantics bit for bit: the fp32 neighbour sum ((E+W)+N)+S and the -4u term contracted into an
// fp32 fma by hipcc, then `0.25*(...) + u` with a double literal, i.e. one fp64 fma on the widened
// values, rounded back to the field type by the store. (E+W == W+E: IEEE addition commutes.)
template <class T>
MDFX_HDI T jacobi5_ref(T c, T xm, T xp, T zm, T zp, T r) {
  const T s = ((xm + xp) + zm) + zp;
  const T t = fmaT(T(-4), c, s);
  return (T)fma((double)r, (double)t, (double)c);
}

// 3D 27-point as a sum of per-plane partials. For one plane and one output column (x, y):
//   center = v(x,y); cross = (v(x-1,y)+v(x+1,y)) + (v(x,y-1)+v(x,y+1));
//   diag   = (v(x-1,y-1)+v(x+1,y-1)) + (v(x-1,y+1)+v(x+1,y+1))
//   A (off-plane contribution) = c3*diag + c2*cross + c1*center
//   B (in-plane contribution)  = c2*diag + c1*cross + c0*center
//   u'(z) = (A(z-1) + B(z)) + A(z+1)
// which equals c0*u + c1*faces(6) + c2*edges(12) + c3*corners(8).
template <class T>
MDFX_HDI T box27_A(T center, T cross, T diag, T c1, T c2, T c3) {
  return fmaT(c3, diag, fmaT(c2, cross, c1 * center));
}
template <class T>
MDFX_HDI T box27_B(T center, T cross, T diag, T c0, T c1, T c2) {
  return fmaT(c2, diag, fmaT(c1, cross, c0 * center));
}
template <class T>
MDFX_HDI T box27_combine(T a_m, T b_c, T a_p) {
  return (a_m + b_c) + a_p;
}

// 2D 9-point (rows are the z axis) as a sum of per-row partials, box27 one dimension down. For one
// row and one column x: c = v(x), h = v(x-1) + v(x+1);
//   A (what the row gives the rows above and below) = c2*h + c1*c
//   B (what the row gives itself)                   = c1*h + c0*c
//   u'(z) = (A(z-1) + B(z)) + A(z+1)
// which equals c0*u + c1*edges(4) + c2*corners(4).
template <class T>
MDFX_HDI T box9_A(T c, T h, T c1, T c2) {
  return fmaT(c2, h, c1 * c);
}
template <class T>
MDFX_HDI T box9_B(T c, T h, T c0, T c1) {
  return fmaT(c1, h, c0 * c);
}
template <class T>
MDFX_HDI T box9_combine(T a_m, T b_c, T a_p) {
  return (a_m + b_c) + a_p;
}

// 3D 7-point star with seven independent weights (star7): a pure chain of one multiply and six fmas,
// ordered for a march along z. For one cell,
//   B  = fma(wyp, yp, fma(wym, ym, fma(wxp, xp, fma(wxm, xm, c0 * c))))   the cell's own plane
//   P  = fma(wzm, zm, B)        complete once plane z has arrived
//   u' = fma(wzp, zp, P)        finished when plane z + 1 arrives
// wxm multiplies u(x-1), wxp multiplies u(x+1); y and z alike.
template <class T>
struct Star7W {
  T c0, xm, xp, ym, yp, zm, zp;
};
template <class T>
MDFX_HDI T star7_B(T c, T xm, T xp, T ym, T yp, T k0, T kxm, T kxp, T kym, T kyp) {
  return fmaT(kyp, yp, fmaT(kym, ym, fmaT(kxp, xp, fmaT(kxm, xm, k0 * c))));
}
template <class T>
MDFX_HDI T star7_P(T B, T zm, T kzm) {
  return fmaT(kzm, zm, B);
}
template <class T>
MDFX_HDI T star7_finish(T P, T zp, T kzp) {
  return fmaT(kzp, zp, P);
}
template <class T>
MDFX_HDI T star7(T c, T xm, T xp, T ym, T yp, T zm, T zp, const Star7W<T>& w) {
  const T B = star7_B<T>(c, xm, xp, ym, yp, w.c0, w.xm, w.xp, w.ym, w.yp);
  return star7_finish<T>(star7_P<T>(B, zm, w.zm), zp, w.zp);
}

// 3D radius-2 star (star13; the fourth-order Laplacian's points): a pure chain of one multiply and twelve
// fmas, ordered for a march along z. c1 weighs the six neighbours at distance 1, c2 the six at distance 2.
// For one cell,
//   B  = the cell's own plane: c0 * c, then fmas of x-1, x+1 (c1), x-2, x+2 (c2), y-1, y+1 (c1), y-2, y+2 (c2)
//   P  = fma(c1, u(z-1), fma(c2, u(z-2), B))   complete once plane z has arrived
//   Q  = fma(c1, u(z+1), P)                    when plane z + 1 arrives
//   u' = fma(c2, u(z+2), Q)                    finished when plane z + 2 arrives
// so the z terms enter in the order the planes pass: z-2, z-1, z+1, z+2.
template <class T>
struct Star13W {
  T c0, c1, c2;
};
template <class T>
MDFX_HDI T star13_B(T c, T xm1, T xp1, T xm2, T xp2, T ym1, T yp1, T ym2, T yp2, const Star13W<T>& w) {
  const T bx = fmaT(w.c2, xp2, fmaT(w.c2, xm2, fmaT(w.c1, xp1, fmaT(w.c1, xm1, w.c0 * c))));
  return fmaT(w.c2, yp2, fmaT(w.c2, ym2, fmaT(w.c1, yp1, fmaT(w.c1, ym1, bx))));
}
template <class T>
MDFX_HDI T star13_P(T B, T zm2, T zm1, const Star13W<T>& w) {
  return fmaT(w.c1, zm1, fmaT(w.c2, zm2, B));
}
template <class T>
MDFX_HDI T star13_zp1(T P, T zp1, const Star13W<T>& w) {
  return fmaT(w.c1, zp1, P);
}
template <class T>
MDFX_HDI T star13_zp2(T Q, T zp2, const Star13W<T>& w) {
  return fmaT(w.c2, zp2, Q);
}
template <class T>
MDFX_HDI T star13(T c, T xm1, T xp1, T xm2, T xp2, T ym1, T yp1, T ym2, T yp2, T zm2, T zm1, T zp1, T zp2,
                  const Star13W<T>& w) {
  const T B = star13_B<T>(c, xm1, xp1, xm2, xp2, ym1, yp1, ym2, yp2, w);
  return star13_zp2<T>(star13_zp1<T>(star13_P<T>(B, zm2, zm1, w), zp1, w), zp2, w);
}

// 2D 9-point with nine independent weights (conv9; rows are the z axis), ordered for a march over rows.
// w is row-major: w[3*(dz+1) + (dx+1)] multiplies u(z+dz, x+dx). An arriving row p with c = v(x),
// l = v(x-1), r = v(x+1) yields three horizontal sums, each one multiply and two fmas:
//   T(p) = fma(w2, r, fma(w0, l, w1 * c))   what row p gives output row p + 1 (it is that row's dz = -1)
//   M(p) = fma(w5, r, fma(w3, l, w4 * c))   what row p gives itself
//   B(p) = fma(w8, r, fma(w6, l, w7 * c))   what row p gives output row p - 1 (that row's dz = +1)
//   u'(z) = (T(z-1) + M(z)) + B(z+1)
template <class T>
struct Conv9W {
  T w[9];  // row-major, in the field type
};
template <class T>
MDFX_HDI T conv9_row(T c, T l, T r, T wl, T wc, T wr) {
  return fmaT(wr, r, fmaT(wl, l, wc * c));
}
template <class T>
MDFX_HDI T conv9_combine(T t_m, T m_c, T b_p) {
  return (t_m + m_c) + b_p;
}
// one cell from its 3x3 neighbourhood: zm / zc / zp point at v(x) of rows z-1 / z / z+1
template <class T>
MDFX_HDI T conv9(const T* zm, const T* zc, const T* zp, const T* w) {
  const T t = conv9_row<T>(zm[0], zm[-1], zm[1], w[0], w[1], w[2]);
  const T m = conv9_row<T>(zc[0], zc[-1], zc[1], w[3], w[4], w[5]);
  const T b = conv9_row<T>(zp[0], zp[-1], zp[1], w[6], w[7], w[8]);
  return conv9_combine<T>(t, m, b);
}

// Life: T = sum of the 3x3 block including self.
MDFX_HDI unsigned char life_rule(unsigned t, unsigned char alive) {
  return (unsigned char)((t == 3u) | ((t == 4u) & (alive != 0)));
}

// Any outer-totalistic Moore rule: bit n of `birth` / `survive` decides a dead / live cell with n
// live neighbours (n = t - alive, 0..8). life_like(t, a, 0x008, 0x00C) == life_rule(t, a).
MDFX_HDI unsigned char life_like(unsigned t, unsigned char alive, unsigned birth, unsigned survive) {
  const unsigned a = alive != 0;
  return (unsigned char)(((a ? survive : birth) >> (t - a)) & 1u);
}

// A Generations rule (B/S/C) with `states` = C cell states, 2 .. 256: n is the number of the eight
// neighbours whose state is exactly 1; s the cell's own state (0 dead, 1 alive, 2 .. C-1 dying).
// life_gen(n, s, b, v, 2) == life_like(n + s, s, b, v) for s in {0, 1}.
MDFX_HDI unsigned char life_gen(unsigned n, unsigned char s, unsigned birth, unsigned survive, unsigned states) {
  if (s == 0) return (unsigned char)((birth >> n) & 1u);
  if (s == 1) return (unsigned char)(((survive >> n) & 1u) ? 1u : 2u % states);
  return (unsigned char)((s + 1u) % states);
}

}  // namespace sm
}  // namespace mdfx
