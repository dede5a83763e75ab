// gpsat_kfun_f64.h -- the covariance functions in fp64, for the fp64 tile kernels and the sparse experts.
// Included inside each kernel file's namespace (under namespace gpsat).
// r2 is the squared scaled distance: kf = k(r) and gg with dk/dl_d = gg (x_d - x'_d)^2 / l_d^3, both without the variance
// factor.
#ifndef GPSAT_KFUN_F64_H
#define GPSAT_KFUN_F64_H

template <int KERN>
__device__ __forceinline__ void kfun(double r2, double& kf, double& gg) {
    if (KERN == 0) {
        kf = exp(-0.5 * r2);
        gg = kf;
    } else {
        const double r = sqrt(fmax(r2, 1e-36));
        if (KERN == 1) {
            kf = exp(-r);
            gg = kf / r;
        } else if (KERN == 2) {
            const double s = 1.7320508075688772 * r, e = exp(-s);
            kf = (1.0 + s) * e;
            gg = 3.0 * e;
        } else {
            const double s = 2.23606797749979 * r, e = exp(-s);
            kf = (1.0 + s + s * s * (1.0 / 3.0)) * e;
            gg = (5.0 / 3.0) * (1.0 + s) * e;
        }
    }
}

// hh = -2 dgg/d(r2), the radial factor of the second derivatives d2k/dx_a dx_b = hh d_a d_b / (l_a l_b) - delta_ab gg / l_a^2
// (d = (x' - x) / l), without the variance factor; for the kernels whose sample paths have a mean-square second derivative:
// KERN 0 (RBF) and 3 (Matern-5/2).  hh(0) = 1 and 25/3.
template <int KERN>
__device__ __forceinline__ double kfun_hh(double r2) {
    static_assert(KERN == 0 || KERN == 3, "hh exists for RBF and Matern-5/2 only");
    // (the exponentials are written as kfun writes them)
    if (KERN == 0) return exp(-0.5 * r2);
    const double r = sqrt(fmax(r2, 1e-36));
    const double s = 2.23606797749979 * r, e = exp(-s);
    return (25.0 / 3.0) * e;
}

#endif
