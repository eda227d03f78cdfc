// nmpc_probe.hip — test-only probe of nmpc_model.h, the Van de Vusse state derivative and RK4 map of the
// NMPC kernel with their forward tangents (the header is included unmodified, with mpct_dev.h and wave_ops.h
// behind it).  The extern "C" entries take host pointers, validate their arguments, allocate, copy, launch
// one 64-thread workgroup per case, synchronise, copy back, free and return the HIP error code.  Built into
// tests/device_units/libmpct_nmpc_probe.so by __graft_entry__.build_nmpc_probe(); never linked into
// libmpct.so.  tests/test_nmpc_units_gpu.py is the only caller.
//
// A case: the parameter row p [16] (mpct.nmpc.VDV_PARAMS order), the state x [3], the inputs u [2], the
// sub-step h and the sub-step count nsub, all wave-uniform as in the kernel, and one tangent seed per lane
// (xd [64][3], ud [64][2]).  Out: what every lane returned, [64][3] values and [64][3] tangents (the tangent
// output of a TAN = false call stays as the caller filled it).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "nmpc_model.h"

using namespace mpct;

namespace {

template <bool RK4, bool TAN>
__global__ void __launch_bounds__(64) nmpc_model_kernel(const double* __restrict__ p, const double* __restrict__ x,
                                                        const double* __restrict__ u, const double* __restrict__ h,
                                                        const int* __restrict__ nsub, const double* __restrict__ xd,
                                                        const double* __restrict__ ud, double* __restrict__ out,
                                                        double* __restrict__ outd) {
  const int lane = threadIdx.x, c = blockIdx.x;
  const VdV P = vdv_load(p + c * NM_NPAR);
  double xs[3] = {x[c * 3], x[c * 3 + 1], x[c * 3 + 2]};
  const double us[2] = {u[c * 2], u[c * 2 + 1]};
  const long long l = (long long)c * 64 + lane;
  double td[3] = {xd[l * 3], xd[l * 3 + 1], xd[l * 3 + 2]};
  const double tu[2] = {ud[l * 2], ud[l * 2 + 1]};
  if (RK4) {
    vdv_rk4<TAN>(P, h[c], nsub[c], xs, us, TAN ? td : nullptr, TAN ? tu : nullptr);
    for (int i = 0; i < 3; ++i) out[l * 3 + i] = xs[i];
    if (TAN)
      for (int i = 0; i < 3; ++i) outd[l * 3 + i] = td[i];
  } else {
    double f[3], fd[3] = {0.0, 0.0, 0.0};
    vdv_rhs<TAN>(P, xs, us, td, tu, f, fd);
    for (int i = 0; i < 3; ++i) out[l * 3 + i] = f[i];
    if (TAN)
      for (int i = 0; i < 3; ++i) outd[l * 3 + i] = fd[i];
  }
}

// device copies of the arguments, freed on every path
struct Arena {
  std::vector<void*> ptrs;
  hipError_t err = hipSuccess;
  ~Arena() {
    for (void* q : ptrs) (void)hipFree(q);
  }
  template <class T>
  T* up(const T* host, size_t n) {
    if (err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, n * sizeof(T));
    if (err != hipSuccess) return nullptr;
    ptrs.push_back(d);
    err = hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice);
    return static_cast<T*>(d);
  }
  template <class T>
  void down(T* host, const T* dev, size_t n) {
    if (err == hipSuccess) err = hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost);
  }
};

int run(bool rk4, int tan, int ncase, const double* p, const double* x, const double* u, const double* h,
        const int* nsub, const double* xd, const double* ud, double* out, double* outd) {
  if ((tan != 0 && tan != 1) || ncase < 1 || ncase > 4096 || !p || !x || !u || !xd || !ud || !out || !outd)
    return (int)hipErrorInvalidValue;
  std::vector<double> h1(ncase, 0.0);
  std::vector<int> n1(ncase, 1);
  if (rk4) {
    if (!h || !nsub) return (int)hipErrorInvalidValue;
    for (int c = 0; c < ncase; ++c) {
      if (!(h[c] > 0.0) || !std::isfinite(h[c]) || nsub[c] < 1 || nsub[c] > 1000) return (int)hipErrorInvalidValue;
      h1[c] = h[c];
      n1[c] = nsub[c];
    }
  }
  for (int c = 0; c < ncase; ++c) {  // the divisions of vdv_load
    const double* q = p + (size_t)c * NM_NPAR;
    if (q[NM_RHO] * q[NM_CP] * q[NM_V] == 0.0) return (int)hipErrorInvalidValue;
  }
  const size_t n = (size_t)ncase;
  Arena A;
  const double* dp = A.up(p, n * NM_NPAR);
  const double* dx = A.up(x, n * 3);
  const double* du = A.up(u, n * 2);
  const double* dh = A.up(h1.data(), n);
  const int* dn = A.up(n1.data(), n);
  const double* dxd = A.up(xd, n * 64 * 3);
  const double* dud = A.up(ud, n * 64 * 2);
  double* dout = A.up(out, n * 64 * 3);
  double* doutd = A.up(outd, n * 64 * 3);
  if (A.err != hipSuccess) return (int)A.err;
  if (rk4 && tan)
    nmpc_model_kernel<true, true><<<ncase, 64>>>(dp, dx, du, dh, dn, dxd, dud, dout, doutd);
  else if (rk4)
    nmpc_model_kernel<true, false><<<ncase, 64>>>(dp, dx, du, dh, dn, dxd, dud, dout, doutd);
  else if (tan)
    nmpc_model_kernel<false, true><<<ncase, 64>>>(dp, dx, du, dh, dn, dxd, dud, dout, doutd);
  else
    nmpc_model_kernel<false, false><<<ncase, 64>>>(dp, dx, du, dh, dn, dxd, dud, dout, doutd);
  A.err = hipGetLastError();
  if (A.err == hipSuccess) A.err = hipDeviceSynchronize();
  if (A.err != hipSuccess) return (int)A.err;
  A.down(out, dout, n * 64 * 3);
  A.down(outd, doutd, n * 64 * 3);
  return (int)A.err;
}

}  // namespace

extern "C" {

// vdv_rhs<tan>: p [ncase][16], x [ncase][3], u [ncase][2], xd [ncase][64][3], ud [ncase][64][2];
// f, fd [ncase][64][3]
int probe_vdv_rhs(int tan, int ncase, const double* p, const double* x, const double* u, const double* xd,
                  const double* ud, double* f, double* fd) {
  return run(false, tan, ncase, p, x, u, nullptr, nullptr, xd, ud, f, fd);
}

// vdv_rk4<tan>: also h [ncase] (> 0) and nsub [ncase] (1..1000); xout, xdout [ncase][64][3]
int probe_vdv_rk4(int tan, int ncase, const double* p, const double* x, const double* u, const double* h,
                  const int* nsub, const double* xd, const double* ud, double* xout, double* xdout) {
  return run(true, tan, ncase, p, x, u, h, nsub, xd, ud, xout, xdout);
}

}  // extern "C"
