// sfw_math_probe.hip — test-only: one element-wise kernel per function of csrc/sfw_math.h, so that tests/test_device_math_gpu.py
// can hold the device math to high-precision references on its own terms (the product's tests see it only through whole
// rollouts).  Includes sfw_math.h and nothing else of the product.  Built twice by `make -C csrc mathprobe`: with the default
// polynomial degrees and with -DSFW_ASIN_DEG=8 -DSFW_EXP_DEG=9 (the degrees of the strict K2 build).
//
// Every kernel: 64-thread blocks, one element per thread, `t < n` guard, and — as every K2 kernel of the product, whatever its
// force type — fp_mode_for_omod() as its first statement (rsqrt_sqrt(double)'s Newton step depends on it).
// Every entry: host pointers and n in, allocate, copy, launch, synchronise, copy back, free; returns the hipError_t as an int
// (0 = hipSuccess); whatever was allocated is freed on every path.
#include "../../social_force_window_planner_amd/csrc/sfw_math.h"

#include <cstddef>

namespace {

constexpr int kBlock = 64;

template <typename R> __global__ void __launch_bounds__(kBlock) k_rsqrt_sqrt(const R *x, R *rs, R *sq, int n) {
  sfwm::fp_mode_for_omod();
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t < n) {
    R a, b;
    sfwm::rsqrt_sqrt(x[t], a, b);
    rs[t] = a;
    sq[t] = b;
  }
}
template <typename R> __global__ void __launch_bounds__(kBlock) k_rcp_nr(const R *x, R *out, int n) {
  sfwm::fp_mode_for_omod();
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t < n) out[t] = sfwm::rcp_nr(x[t]);
}
template <typename R> __global__ void __launch_bounds__(kBlock) k_exp2_fast(const R *x, R *out, int n) {
  sfwm::fp_mode_for_omod();
  const sfwm::poly_consts pc;
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t < n) out[t] = sfwm::exp2_fast(pc, x[t]);
}
template <typename R> __global__ void __launch_bounds__(kBlock) k_exp2_scaled(const R *u, const R *c, R *out, int n) {
  sfwm::fp_mode_for_omod();
  const sfwm::poly_consts pc;
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t < n) out[t] = sfwm::exp2_scaled(pc, u[t], c[t]);
}
template <typename R>
__global__ void __launch_bounds__(kBlock) k_exp2_fast2_gated(const R *x1, const R *x2, const double *cw, R *e1, R *e2, int n) {
  sfwm::fp_mode_for_omod();
  const sfwm::poly_consts pc;
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t < n) {
    R a, b;
    sfwm::exp2_fast2_gated(pc, x1[t], x2[t], cw[t], a, b);
    e1[t] = a;
    e2[t] = b;
  }
}
template <typename R>
__global__ void __launch_bounds__(kBlock) k_angle_abs(const R *y, const R *nx, const R *rh, const R *hyp, R *out, int n) {
  sfwm::fp_mode_for_omod();
  const sfwm::poly_consts pc;
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t < n) out[t] = sfwm::angle_abs(pc, y[t], nx[t], rh[t], hyp[t]);
}
// rh and hyp from the device's own root of nx^2 + y^2, formed as pair_force forms its norms
__global__ void __launch_bounds__(kBlock) k_angle_abs_composed(const double *y, const double *nx, double *out, int n) {
  sfwm::fp_mode_for_omod();
  const sfwm::poly_consts pc;
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t < n) {
    double rh, hyp;
    sfwm::rsqrt_sqrt(fma(nx[t], nx[t], y[t] * y[t]), rh, hyp);
    out[t] = sfwm::angle_abs(pc, y[t], nx[t], rh, hyp);
  }
}

// The device copies of one call: NI inputs, then NO outputs, each n elements of its own size.  The destructor frees
// whatever was allocated, on the failing paths too.
struct device_bufs {
  static constexpr int kMax = 8;
  void *p[kMax] = {};
  ~device_bufs() {
    for (void *q : p)
      if (q) (void)hipFree(q);
  }
};
struct host_array {
  void *ptr;
  size_t elem;
  bool output;
};
template <typename Launch> int run(const host_array *a, int count, int n, Launch launch) {
  if (n <= 0 || count > device_bufs::kMax) return static_cast<int>(hipErrorInvalidValue);
  for (int i = 0; i < count; ++i)
    if (!a[i].ptr) return static_cast<int>(hipErrorInvalidValue);
  device_bufs d;
  hipError_t e;
  for (int i = 0; i < count; ++i) {
    const size_t bytes = a[i].elem * static_cast<size_t>(n);
    if ((e = hipMalloc(&d.p[i], bytes)) != hipSuccess) {
      d.p[i] = nullptr;
      return static_cast<int>(e);
    }
    if (!a[i].output && (e = hipMemcpy(d.p[i], a[i].ptr, bytes, hipMemcpyHostToDevice)) != hipSuccess) return static_cast<int>(e);
  }
  launch(d.p, dim3((n + kBlock - 1) / kBlock), dim3(kBlock));
  if ((e = hipGetLastError()) != hipSuccess) return static_cast<int>(e);
  if ((e = hipDeviceSynchronize()) != hipSuccess) return static_cast<int>(e);
  for (int i = 0; i < count; ++i)
    if (a[i].output && (e = hipMemcpy(a[i].ptr, d.p[i], a[i].elem * static_cast<size_t>(n), hipMemcpyDeviceToHost)) != hipSuccess)
      return static_cast<int>(e);
  return static_cast<int>(hipSuccess);
}
template <typename T> host_array in(const T *p) { return {const_cast<T *>(p), sizeof(T), false}; }
template <typename T> host_array out(T *p) { return {p, sizeof(T), true}; }
template <typename T> T *as(void *p) { return static_cast<T *>(p); }

template <typename R> int rsqrt_sqrt(const R *x, R *rs, R *sq, int n) {
  const host_array a[] = {in(x), out(rs), out(sq)};
  return run(a, 3, n, [n](void **d, dim3 g, dim3 b) { hipLaunchKernelGGL(k_rsqrt_sqrt<R>, g, b, 0, 0, as<R>(d[0]), as<R>(d[1]), as<R>(d[2]), n); });
}
template <typename R> int rcp_nr(const R *x, R *o, int n) {
  const host_array a[] = {in(x), out(o)};
  return run(a, 2, n, [n](void **d, dim3 g, dim3 b) { hipLaunchKernelGGL(k_rcp_nr<R>, g, b, 0, 0, as<R>(d[0]), as<R>(d[1]), n); });
}
template <typename R> int exp2_fast(const R *x, R *o, int n) {
  const host_array a[] = {in(x), out(o)};
  return run(a, 2, n, [n](void **d, dim3 g, dim3 b) { hipLaunchKernelGGL(k_exp2_fast<R>, g, b, 0, 0, as<R>(d[0]), as<R>(d[1]), n); });
}
template <typename R> int exp2_scaled(const R *u, const R *c, R *o, int n) {
  const host_array a[] = {in(u), in(c), out(o)};
  return run(a, 3, n, [n](void **d, dim3 g, dim3 b) { hipLaunchKernelGGL(k_exp2_scaled<R>, g, b, 0, 0, as<R>(d[0]), as<R>(d[1]), as<R>(d[2]), n); });
}
template <typename R> int exp2_fast2_gated(const R *x1, const R *x2, const double *cw, R *e1, R *e2, int n) {
  const host_array a[] = {in(x1), in(x2), in(cw), out(e1), out(e2)};
  return run(a, 5, n, [n](void **d, dim3 g, dim3 b) {
    hipLaunchKernelGGL(k_exp2_fast2_gated<R>, g, b, 0, 0, as<R>(d[0]), as<R>(d[1]), as<double>(d[2]), as<R>(d[3]), as<R>(d[4]), n);
  });
}
template <typename R> int angle_abs(const R *y, const R *nx, const R *rh, const R *hyp, R *o, int n) {
  const host_array a[] = {in(y), in(nx), in(rh), in(hyp), out(o)};
  return run(a, 5, n, [n](void **d, dim3 g, dim3 b) {
    hipLaunchKernelGGL(k_angle_abs<R>, g, b, 0, 0, as<R>(d[0]), as<R>(d[1]), as<R>(d[2]), as<R>(d[3]), as<R>(d[4]), n);
  });
}

}  // namespace

extern "C" {
// the build's polynomial degrees and whether the Newton step of the root uses the output modifier
void probe_config(int *asin_deg, int *exp_deg, int *omod) {
  *asin_deg = SFW_ASIN_DEG;
  *exp_deg = SFW_EXP_DEG;
  *omod = SFW_OMOD;
}
int probe_rsqrt_sqrt_f64(const double *x, double *rs, double *sq, int n) { return rsqrt_sqrt(x, rs, sq, n); }
int probe_rcp_nr_f64(const double *x, double *o, int n) { return rcp_nr(x, o, n); }
int probe_exp2_fast_f64(const double *x, double *o, int n) { return exp2_fast(x, o, n); }
int probe_exp2_scaled_f64(const double *u, const double *c, double *o, int n) { return exp2_scaled(u, c, o, n); }
int probe_exp2_fast2_gated_f64(const double *x1, const double *x2, const double *cw, double *e1, double *e2, int n) {
  return exp2_fast2_gated(x1, x2, cw, e1, e2, n);
}
int probe_angle_abs_f64(const double *y, const double *nx, const double *rh, const double *hyp, double *o, int n) {
  return angle_abs(y, nx, rh, hyp, o, n);
}
int probe_angle_abs_composed_f64(const double *y, const double *nx, double *o, int n) {
  const host_array a[] = {in(y), in(nx), out(o)};
  return run(a, 3, n, [n](void **d, dim3 g, dim3 b) {
    hipLaunchKernelGGL(k_angle_abs_composed, g, b, 0, 0, as<double>(d[0]), as<double>(d[1]), as<double>(d[2]), n);
  });
}
int probe_rsqrt_sqrt_f32(const float *x, float *rs, float *sq, int n) { return rsqrt_sqrt(x, rs, sq, n); }
int probe_rcp_nr_f32(const float *x, float *o, int n) { return rcp_nr(x, o, n); }
int probe_exp2_fast_f32(const float *x, float *o, int n) { return exp2_fast(x, o, n); }
int probe_exp2_scaled_f32(const float *u, const float *c, float *o, int n) { return exp2_scaled(u, c, o, n); }
int probe_exp2_fast2_gated_f32(const float *x1, const float *x2, const double *cw, float *e1, float *e2, int n) {
  return exp2_fast2_gated(x1, x2, cw, e1, e2, n);
}
int probe_angle_abs_f32(const float *y, const float *nx, const float *rh, const float *hyp, float *o, int n) {
  return angle_abs(y, nx, rh, hyp, o, n);
}
}
