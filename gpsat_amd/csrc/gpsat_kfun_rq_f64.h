// gpsat_kfun_rq_f64.h -- the RationalQuadratic covariance function in fp64, KN == 4 of the fp64 tile kernel (instantiated in
// its rq variant only).  Included inside the kernel file's namespace (under namespace gpsat), like gpsat_kfun_f64.h.
//   k = s b^-alpha,  b = 1 + r2 / (2 alpha),  r2 the squared scaled distance   (GPflow's and scikit-learn's RationalQuadratic)
// a = alpha, ha = 1 / (2 alpha).  Out, all without the variance factor s: kf = k, gg with dk/dl_d = gg (x_d - x'_d)^2 / l_d^3
// (gg = kf / b), and ga = dk/dalpha = kf (-log b + (b - 1) / b).  r2 = 0 gives kf = 1 and ga = 0 exactly.
#ifndef GPSAT_KFUN_RQ_F64_H
#define GPSAT_KFUN_RQ_F64_H

__device__ __forceinline__ void kfun_rq(double a, double ha, double r2, double& kf, double& gg, double& ga) {
    const double x = r2 * ha;                  // b - 1
    const double lb = log1p(x);
    const double ib = 1.0 / (1.0 + x);
    kf = exp(-a * lb);
    gg = kf * ib;
    ga = kf * (x * ib - lb);
}

#endif
