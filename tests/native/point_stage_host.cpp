// Array forms of the per-point functions of csrc/nsc_math.h for the host (test tool, built by
// tests/point_families.py with g++ -O2 -ffp-contract=off -shared -fPIC, once plain and once each with
// -DNSC_TEST_APPROX_BIAS=1 / =-1, which push the 1-ULP error of v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 to either side).
//   psh_make_bin_params   nsc_make_bin_params(): the struct itself, so that tests read narrow_fov, simple_valid, s_lo, s_hi
//   psh_point_lean        nsc_point_lean():  status 0 = dropped, 1 = certain, 2 = uncertain; pixel; squared range
//   psh_point_pixel       nsc_point_pixel(): flags 0 = dropped, else 1 | 2 (column exact) | 4 (row exact); pixel; squared range
//   psh_point_exact       nsc_point_exact() where keep[i] != 0, -1 elsewhere
#include <cstdint>
#include "nsc_math.h"

extern "C" {

int psh_bias(void)
{
#if defined(NSC_TEST_APPROX_BIAS)
    return NSC_TEST_APPROX_BIAS;
#else
    return 0;
#endif
}

int psh_sizeof_bin_params(void) { return (int)sizeof(NscBinParams); }

float psh_az_edge_slack(void) { return nsc_az_edge_slack(); }

int psh_make_bin_params(int E, double emin, double emax, float rmin, float rmax, int elev_f64, NscBinParams *out)
{
    *out = nsc_make_bin_params(E, emin, emax, rmin, rmax, elev_f64);
    return nsc_lean_ok(*out) ? 1 : 0;
}

void psh_point_lean(const float *pts, int64_t n, int stride, const NscBinParams *bp, int32_t *status, int32_t *pix, float *s)
{
    for (int64_t i = 0; i < n; ++i) {
        int p = -1; float sv = 0.0f;
        status[i] = nsc_point_lean(pts[i * stride], pts[i * stride + 1], pts[i * stride + 2], *bp, p, sv);
        pix[i] = status[i] ? p : -1;
        s[i] = sv;
    }
}

void psh_point_pixel(const float *pts, int64_t n, int stride, const NscBinParams *bp, int32_t *flags, int32_t *pix, float *s)
{
    for (int64_t i = 0; i < n; ++i) {
        int p = -1; float sv = 0.0f;
        flags[i] = nsc_point_pixel(pts[i * stride], pts[i * stride + 1], pts[i * stride + 2], *bp, p, sv);
        pix[i] = flags[i] ? p : -1;
        s[i] = sv;
    }
}

void psh_point_exact(const float *pts, int64_t n, int stride, const NscBinParams *bp, const uint8_t *keep, int32_t *pix)
{
    for (int64_t i = 0; i < n; ++i)
        pix[i] = keep[i] ? nsc_point_exact(pts[i * stride], pts[i * stride + 1], pts[i * stride + 2], *bp) : -1;
}

}  // extern "C"
