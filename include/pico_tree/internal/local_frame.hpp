// local_frame.hpp -- normals_within_self (ptk.h): the moments of a point's neighbourhood, their covariance
// and the local frame (normal, curvature, eigenvalues) of that covariance, as the contract reads.  ONE routine: compiled
// for the device by frames_self_kernel (pico_tree_amd/csrc/ptk_kernels_frames.hpp), for the library's host loop
// (ptk_host_normals_within_self) and for kd_tree::normals_within_self where the backend does not serve.
//
// Every operation is an IEEE float32 + - * / or sqrtf, each rounded once, in the order written: the units that include
// this header are compiled with -ffp-contract=off (a fused multiply-add would change the bits), and the frame is then a
// function of the bits of the covariance -- the same on the device and on the host.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PICO_TREE_HD __host__ __device__
#else
#define PICO_TREE_HD
#endif

namespace pico_tree::internal {

//! ptk_moments (ptk.h): 48 bytes.
struct moments3 {
  float sum[3];
  std::uint32_t count;
  float outer[6];  // xx, xy, xz, yy, yz, zz
  std::uint32_t pad_[2];
};
//! ptk_frame (ptk.h): 32 bytes.
struct frame3 {
  float normal[3];
  float curvature;
  float eigenvalues[3];
  std::uint32_t count;
};
static_assert(sizeof(moments3) == 48 && sizeof(frame3) == 32, "record layout");

//! The running sums of one row: every accumulator starts at +0 and takes the offsets in row order.
struct moment_sums {
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  float xx = 0.0f, xy = 0.0f, xz = 0.0f, yy = 0.0f, yz = 0.0f, zz = 0.0f;
  std::uint32_t count = 0;

  //! One accepted neighbour at offset u = p_i - p_j (query first).
  PICO_TREE_HD inline void add(float ux, float uy, float uz) {
    sx = sx + ux;
    sy = sy + uy;
    sz = sz + uz;
    xx = xx + ux * ux;
    xy = xy + ux * uy;
    xz = xz + ux * uz;
    yy = yy + uy * uy;
    yz = yz + uy * uz;
    zz = zz + uz * uz;
    ++count;
  }

  PICO_TREE_HD inline moments3 record() const {
    moments3 m;
    m.sum[0] = sx, m.sum[1] = sy, m.sum[2] = sz;
    m.count = count;
    m.outer[0] = xx, m.outer[1] = xy, m.outer[2] = xz, m.outer[3] = yy, m.outer[4] = yz, m.outer[5] = zz;
    m.pad_[0] = m.pad_[1] = 0;
    return m;
  }
};

PICO_TREE_HD inline float frame_nan() {
  std::uint32_t const bits = 0x7FC00000u;
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __uint_as_float(bits);
#else
  std::memcpy(&f, &bits, sizeof f);
#endif
  return f;
}

PICO_TREE_HD inline bool frame_finite(float x) { return x - x == 0.0f; }

//! C (xx, xy, xz, yy, yz, zz) of the sums: the point itself belongs to its neighbourhood with offset 0, so the divisor is
//! count + 1.
PICO_TREE_HD inline void covariance_of(moment_sums const& s, float c[6]) {
  float const m = static_cast<float>(s.count + 1u);
  float const inv = 1.0f / m;
  float const mx = s.sx * inv, my = s.sy * inv, mz = s.sz * inv;
  c[0] = s.xx * inv - mx * mx;
  c[1] = s.xy * inv - mx * my;
  c[2] = s.xz * inv - mx * mz;
  c[3] = s.yy * inv - my * my;
  c[4] = s.yz * inv - my * mz;
  c[5] = s.zz * inv - mz * mz;
}

//! One Jacobi rotation of the symmetric 3 x 3 in the plane (p, q), r being the third index: app, aqq the diagonal
//! entries, apq the element to annihilate, arp, arq the other two; (v0p, v0q) ... the columns p and q of the eigenvector
//! matrix.  An off-diagonal element that is exactly 0 is skipped.
PICO_TREE_HD inline void jacobi_rotate(
    float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p, float& v0q, float& v1p, float& v1q, float& v2p,
    float& v2q) {
  if (apq == 0.0f) return;
  float const theta = (aqq - app) / (2.0f * apq);
  float const mag = theta < 0.0f ? -theta : theta;
  float const root = sqrtf(theta * theta + 1.0f);
  float const tm = 1.0f / (mag + root);
  float const t = theta < 0.0f ? -tm : tm;
  float const c = 1.0f / sqrtf(t * t + 1.0f);
  float const s = t * c;
  float const tau = s / (1.0f + c);
  float const h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0f;
  float const g = arp, k = arq;
  arp = g - s * (k + tau * g);
  arq = k + s * (g - tau * k);
  float const a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = a0 - s * (b0 + tau * a0);
  v0q = b0 + s * (a0 - tau * b0);
  v1p = a1 - s * (b1 + tau * a1);
  v1q = b1 + s * (a1 - tau * b1);
  v2p = a2 - s * (b2 + tau * a2);
  v2q = b2 + s * (a2 - tau * b2);
}

//! The frame of the sums of point (px, py, pz).  `view` null: the normal's component of largest magnitude is made
//! positive (ties: x, then y, then z); else the normal is turned towards the viewpoint.
PICO_TREE_HD inline frame3 frame_of(
    moment_sums const& sums, std::uint64_t min_neighbors, bool has_view, float vx, float vy, float vz, float px, float py,
    float pz) {
  frame3 f;
  f.count = sums.count;
  float c[6];
  covariance_of(sums, c);
  std::uint64_t const need = min_neighbors > 2u ? min_neighbors : 2u;  // (a plane needs three points)
  bool finite = true;
  for (int a = 0; a < 6; ++a) finite = finite && frame_finite(c[a]);
  if (sums.count < need || !finite) {
    float const nan = frame_nan();
    f.normal[0] = f.normal[1] = f.normal[2] = nan;
    f.curvature = nan;
    f.eigenvalues[0] = f.eigenvalues[1] = f.eigenvalues[2] = nan;
    return f;
  }
  // Cyclic Jacobi, a FIXED 6 sweeps over (0,1), (0,2), (1,2): no convergence test, no data-dependent trip count.
  float a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
  float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
  for (int sweep = 0; sweep < 6; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  // Clamped below at +0, then sorted ascending by the fixed network (0,1), (1,2), (0,1); a strict > swaps, so equal
  // values keep their columns.
  float l0 = a00 > 0.0f ? a00 : 0.0f, l1 = a11 > 0.0f ? a11 : 0.0f, l2 = a22 > 0.0f ? a22 : 0.0f;
  float n0x = v00, n0y = v10, n0z = v20;  // column 0
  float n1x = v01, n1y = v11, n1z = v21;
  float n2x = v02, n2y = v12, n2z = v22;
  float tmp;
#define PICO_TREE_FRAME_SWAP(A, B) tmp = A, A = B, B = tmp
  if (l0 > l1) {
    PICO_TREE_FRAME_SWAP(l0, l1);
    PICO_TREE_FRAME_SWAP(n0x, n1x);
    PICO_TREE_FRAME_SWAP(n0y, n1y);
    PICO_TREE_FRAME_SWAP(n0z, n1z);
  }
  if (l1 > l2) {
    PICO_TREE_FRAME_SWAP(l1, l2);
    PICO_TREE_FRAME_SWAP(n1x, n2x);
    PICO_TREE_FRAME_SWAP(n1y, n2y);
    PICO_TREE_FRAME_SWAP(n1z, n2z);
  }
  if (l0 > l1) {
    PICO_TREE_FRAME_SWAP(l0, l1);
    PICO_TREE_FRAME_SWAP(n0x, n1x);
    PICO_TREE_FRAME_SWAP(n0y, n1y);
    PICO_TREE_FRAME_SWAP(n0z, n1z);
  }
#undef PICO_TREE_FRAME_SWAP
  (void)n2x, (void)n2y, (void)n2z;
  float const len = sqrtf((n0x * n0x + n0y * n0y) + n0z * n0z);
  float nx = n0x / len, ny = n0y / len, nz = n0z / len;
  bool flip;
  if (has_view) {
    float const wx = vx - px, wy = vy - py, wz = vz - pz;
    flip = ((nx * wx + ny * wy) + nz * wz) < 0.0f;
  } else {
    float const ax = nx < 0.0f ? -nx : nx, ay = ny < 0.0f ? -ny : ny, az = nz < 0.0f ? -nz : nz;
    float const lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
    flip = lead < 0.0f;
  }
  if (flip) nx = -nx, ny = -ny, nz = -nz;
  f.normal[0] = nx, f.normal[1] = ny, f.normal[2] = nz;
  float const total = (l0 + l1) + l2;
  f.curvature = total == 0.0f ? 0.0f : l0 / total;
  f.eigenvalues[0] = l0, f.eigenvalues[1] = l1, f.eigenvalues[2] = l2;
  return f;
}

//! The host form of one row: the offsets of `row` (entries with .index, in row order, the own entry removed) about point
//! i of `points` (n x 3, row-major).
template <typename Row_>
inline moment_sums sums_of_row(float const* points, std::size_t i, Row_ const& row) {
  moment_sums s;
  float const* p = points + 3 * i;
  for (auto const& nb : row) {
    float const* o = points + 3 * static_cast<std::size_t>(nb.index);
    s.add(p[0] - o[0], p[1] - o[1], p[2] - o[2]);
  }
  return s;
}

}  // namespace pico_tree::internal

namespace pico_tree {

//! The records of kd_tree::normals_within_self (ptk_frame / ptk_moments of ptk.h).
using local_frame = internal::frame3;
using local_moments = internal::moments3;

}  // namespace pico_tree
