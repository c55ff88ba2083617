// bdpt_math.h — the device core's base: host / device function macros (with the host build's
// shims), constants, fp32 3-vectors and frames, the Philox counter RNG, and the fixed-polynomial
// cos / sin / atan2 of the fp32 device semantics.

#pragma once

#include <stdint.h>

#include <type_traits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BDPT_HD __host__ __device__ __forceinline__
#define BDPT_D __device__ __forceinline__
#else
#include <cmath>
#define BDPT_HD inline
#define BDPT_D inline
#include <cstring>
using std::sqrt;
struct float4 {
  float x, y, z, w;
};
inline int __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
inline float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }
#endif

namespace bdpt {

// ------------------------------------------------------------------------------------------------
// Constants (CGL/include/CGL/misc.h:11-14)
#define BDPT_PI_F 3.14159265358979323f
#define BDPT_EPS_F 0.00001f

// ------------------------------------------------------------------------------------------------
// fp32 3-vectors with CGL Vector3D operation order (vector3D.h)
struct f3 {
  float x, y, z;
};
BDPT_HD f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
BDPT_HD f3 add(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
BDPT_HD f3 sub(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
BDPT_HD f3 mul(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
BDPT_HD f3 muls(f3 a, float c) { return mk3(a.x * c, a.y * c, a.z * c); }      // v * c
BDPT_HD f3 smul(float c, f3 a) { return mk3(c * a.x, c * a.y, c * a.z); }      // c * v
BDPT_HD f3 divs(f3 a, float c) { float rc = 1.0f / c; return mk3(rc * a.x, rc * a.y, rc * a.z); }
BDPT_HD f3 neg(f3 a) { return mk3(-a.x, -a.y, -a.z); }
BDPT_HD float dot(f3 u, f3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }
BDPT_HD float norm2(f3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
BDPT_HD float norm(f3 a) { return sqrtf(norm2(a)); }
BDPT_HD f3 normalize(f3 a) { float rc = 1.0f / norm(a); return mk3(a.x * rc, a.y * rc, a.z * rc); }
BDPT_HD f3 cross(f3 u, f3 v) {
  return mk3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}
BDPT_HD f3 splat3(float c) { return mk3(c, c, c); }

// make_coord_space (bsdf.cpp:21-41): columns X, Y, Z of o2w.
struct Frame {
  f3 X, Y, Z;
};
template <bool UNIT = false>
BDPT_HD Frame make_frame_t(f3 n) {
  f3 z = n, h = n;
  if (fabsf(h.x) <= fabsf(h.y) && fabsf(h.x) <= fabsf(h.z)) h.x = 1.0f;
  else if (fabsf(h.y) <= fabsf(h.x) && fabsf(h.y) <= fabsf(h.z)) h.y = 1.0f;
  else h.z = 1.0f;
  if (!UNIT) z = normalize(z);
  f3 y = normalize(cross(h, z));
  f3 x = normalize(cross(z, y));
  Frame f;
  f.X = x; f.Y = y; f.Z = z;
  return f;
}
BDPT_HD Frame make_frame(f3 n) { return make_frame_t<false>(n); }
// The frame of a surface hit. Its shading normal is already normalize()d (shade_hit), so the
// fp32 semantics take Z = n instead of normalising it a second time (which moves a component by
// at most an ulp, in about 1 of 4 normals): one normalize less per vertex, and a stored path
// vertex needs no separate shading axis (oracle mode 2 does the same).
BDPT_HD Frame make_frame_hit(f3 n) { return make_frame_t<true>(n); }
// o2w * v (matrix3x3.cpp:110-114) and w2o * v = o2w.T() * v
BDPT_HD f3 to_world(const Frame& f, f3 v) { return add(add(smul(v.x, f.X), smul(v.y, f.Y)), smul(v.z, f.Z)); }
BDPT_HD float lz(f3 v, f3 Z) { return v.x * Z.x + v.y * Z.y + v.z * Z.z; }   // (w2o*v).z
BDPT_HD f3 to_local(const Frame& f, f3 v) { return mk3(lz(v, f.X), lz(v, f.Y), lz(v, f.Z)); }
BDPT_HD f3 zaxis(f3 n) { return normalize(n); }   // make_coord_space(n).Z without X, Y
BDPT_HD bool nonzero3(f3 v) { return (v.x != 0) | (v.y != 0) | (v.z != 0); }

// ------------------------------------------------------------------------------------------------
// Counter RNG: Philox4x32-10, counter (pixel, sample, block, 0xB1D1), key (seed lo, hi).
// Sub-streams of one pixel-sample (identical in oracle/bdpt_oracle.cpp CounterStream):
// 0 = camera jitter + eye walk, 1 = light choice + light walk, 2 + i = the fresh light sample of
// connection (i, j = 1). Counter = (pixel, sample, block, 0xB1D1 + (stream << 16)), so phases and
// connections can be evaluated in any order and skipped connections consume nothing.
struct Rng {
  uint32_t k0, k1, pix, smp;
  uint32_t pos;   // uniform index within the stream: block = pos >> 2, word = pos & 3
  uint32_t cur;   // block held in b0..b3 (0xffffffff: none)
  uint32_t tag;   // 0xB1D1 + (stream << 16)
  uint32_t b0, b1, b2, b3;
};
BDPT_HD void rng_init(Rng& r, uint64_t seed, uint32_t pixel, uint32_t sample) {
  r.k0 = (uint32_t)seed; r.k1 = (uint32_t)(seed >> 32); r.pix = pixel; r.smp = sample;
  r.pos = 0; r.cur = 0xffffffffu; r.tag = 0xB1D1u;
}
BDPT_HD void rng_stream(Rng& r, uint32_t s) {
  r.pos = 0; r.cur = 0xffffffffu; r.tag = 0xB1D1u + (s << 16);
}
BDPT_HD void philox(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
BDPT_HD float u_of(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }
BDPT_HD float rng_next(Rng& r) {
  const uint32_t blk = r.pos >> 2;
  if (blk != r.cur) {
    r.b0 = r.pix; r.b1 = r.smp; r.b2 = blk; r.b3 = r.tag;
    philox(r.b0, r.b1, r.b2, r.b3, r.k0, r.k1);
    r.cur = blk;
  }
  const uint32_t w = r.pos & 3u;
  uint32_t x = w == 0 ? r.b0 : w == 1 ? r.b1 : w == 2 ? r.b2 : r.b3;
  r.pos++;
  return u_of(x);
}
// Consume n uniforms without using them (a connection whose value is known to be zero still
// advances the stream exactly as the reference's draws would).
BDPT_HD void rng_skip(Rng& r, uint32_t n) { r.pos += n; }

// cos/sin(2*pi*u), u in (0,1): quadrant split + Taylor polynomials (same as the oracle's).
BDPT_HD void cos_sin_2pi(float u, float* c, float* s) {
  float t = u * 4.0f;
  int k = (int)(t + 0.5f);
  float f = u - (float)k * 0.25f;
  float f2 = f * f;
  float sp = f * (6.2831854820251465f +
                  f2 * (-41.34170150756836f +
                        f2 * (81.6052474975586f + f2 * (-76.70585632324219f + f2 * 42.058692932128906f))));
  float cp = 1.0f + f2 * (-19.739208221435547f +
                          f2 * (64.93939208984375f +
                                f2 * (-85.45681762695312f + f2 * (60.2446403503418f + f2 * -26.42625617980957f))));
  int q = k & 3;
  float cc = q == 0 ? cp : q == 1 ? -sp : q == 2 ? -cp : sp;
  float ss = q == 0 ? sp : q == 1 ? cp : q == 2 ? -sp : -cp;
  *c = cc;
  *s = ss;
}

// atan2(y, x) for the environment map's direction -> (theta, phi) (environment_light.cpp:97-102):
// octant reduction + the Cephes atanf polynomial (|err| ~ 1e-7), plain fp32 operations so the
// oracle's mode 2 (oracle/bdpt_oracle.cpp atan2_f32) evaluates it bit-identically.
BDPT_HD float atan2_det(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  if (ax == 0.0f && ay == 0.0f) return 0.0f;
  float t = ay <= ax ? ay / ax : ax / ay;   // [0, 1]
  float off = 0.0f;
  if (t > 0.41421356237309503f) {           // tan(pi/8): atan t = pi/4 + atan((t-1)/(t+1))
    off = 0.78539816339744831f;
    t = (t - 1.0f) / (t + 1.0f);
  }
  const float z = t * t;
  float r = ((((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f) * z) * t + t;
  r = off + r;
  if (ay > ax) r = 1.57079632679489662f - r;
  if (x < 0.0f) r = 3.14159265358979323f - r;
  return y < 0.0f ? -r : r;
}
// lround for x >= 0 (std::lround: halves away from zero), exact: x - floor(x) is exact.
BDPT_HD int lround_pos(float x) {
  const float f = floorf(x);
  return (int)f + ((x - f) >= 0.5f ? 1 : 0);
}

}  // namespace bdpt
