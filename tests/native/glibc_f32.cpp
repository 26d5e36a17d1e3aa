// glibc's float functions over arrays, for the numpy restatements of include/mgym.h (tests/glibc_f32.py): numpy's own float32 sin / cos / tanh are not
// glibc's, and Python 3.10 has no math.fma.  Built with g++ -ffp-contract=off and without -mfma as a shared object, so every call below is the libm call:
// fmaf is ONE correctly rounded operation per element.
#include <cmath>
#include <cstdint>

extern "C" {
void glibc_sinf(uint64_t n, const float* x, float* y) { for (uint64_t i = 0; i < n; ++i) y[i] = sinf(x[i]); }
void glibc_cosf(uint64_t n, const float* x, float* y) { for (uint64_t i = 0; i < n; ++i) y[i] = cosf(x[i]); }
void glibc_tanhf(uint64_t n, const float* x, float* y) { for (uint64_t i = 0; i < n; ++i) y[i] = tanhf(x[i]); }
void glibc_expm1f(uint64_t n, const float* x, float* y) { for (uint64_t i = 0; i < n; ++i) y[i] = expm1f(x[i]); }
void glibc_fmodf(uint64_t n, const float* x, float m, float* y) { for (uint64_t i = 0; i < n; ++i) y[i] = fmodf(x[i], m); }
void glibc_fmaf(uint64_t n, const float* a, const float* b, const float* c, float* y) { for (uint64_t i = 0; i < n; ++i) y[i] = fmaf(a[i], b[i], c[i]); }
}
