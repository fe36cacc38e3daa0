// TEST-ONLY: the root finder and the E6Q3 elimination of csrc/recover_core.h behind C entries for ctypes
// (tests/test_recover_planted.py).  The recovery hides both behind a projection to the nearest rotation; here they
// are held to properties of their own.
#include "../../cvxpnpl_amd/csrc/recover_core.h"

extern "C" {

// p: deg + 1 coefficients, descending; roots_re / roots_im [deg].  Returns the number of roots.
int rs_poly_roots(const double *p, int deg, double *roots_re, double *roots_im)
{
    cvxr::cd z[8];
    const int n = cvxr::poly_roots(p, deg, z);
    for (int i = 0; i < n; ++i) { roots_re[i] = z[i].re; roots_im[i] = z[i].im; }
    return n;
}

// A [rows][10] in the column order [a^2 b^2 c^2 ab ac bc a b c 1]; a, b, c [4].  Returns the number of solutions.
int rs_e6q3(const double *A, int rows, double *a, double *b, double *c)
{
    return cvxr::e6q3(reinterpret_cast<const double (*)[10]>(A), rows, a, b, c);
}

} // extern "C"
