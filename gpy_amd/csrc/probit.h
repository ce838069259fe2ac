// probit.h -- the Bernoulli / probit moment matching's one special function, shared by ep.hip and epdtc.hip.
#pragma once
#include <cmath>

#include "common.h"

// log Phi(z) and phi(z) / Phi(z) over the whole real line from their definitions: for z < 0 through the scaled complementary
// error function, Phi(z) = erfcx(-z / sqrt2) exp(-z^2 / 2) / 2; for z >= 0 through Phi(z) = 1 - erfc(z / sqrt2) / 2
__device__ __forceinline__ void probit_logcdf(double z, double* log_Phi, double* phi_div_Phi) {
    const double rsqrt2 = 0.70710678118654752440, sqrt_2_over_pi = 0.79788456080286535588, rsqrt_2pi = 0.39894228040143267794;
    if (z < 0.0) {
        const double e = erfcx(-z * rsqrt2);
        *log_Phi = log(0.5 * e) - 0.5 * z * z;
        *phi_div_Phi = sqrt_2_over_pi / e;
    } else {
        const double q = -0.5 * erfc(z * rsqrt2);             // Phi - 1
        *log_Phi = log1p(q);
        *phi_div_Phi = rsqrt_2pi * exp(-0.5 * z * z) / (1.0 + q);
    }
}
