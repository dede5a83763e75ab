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

#endif
