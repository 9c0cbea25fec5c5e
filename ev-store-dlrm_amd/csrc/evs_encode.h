// The offline encoders, one definition for the whole-table tool (evs_encode.hip) and the row-update kernels
// (evs_update.h): fp32 -> the reference's reduced-precision codes, bit-exact with script/reduce_precision.py +
// script/convert_ev_to_binary.py:
//   u8   round(((x + 1) / 2) * 254), Python round = half-to-even            (reduce_precision.py:270)
//   u16  convert_ev_float_to_ushort: linear code inside +-0.65, 0.01 steps with a sign-parity
//        convention outside, int() truncates toward zero                     (reduce_precision.py:26-51)
//   u4   convert_to_4bit_int_posit thresholds, dim 2j in the HIGH nibble    (reduce_precision.py:140-172,321)
// The reference computes in Python floats (doubles) from the CSV text of the fp32 weights; the kernels widen
// the fp32 input to fp64 and do the same IEEE arithmetic (the library is built with -ffp-contract=off).
// Codes are stored like numpy's astype(uint8/uint16): modulo 2^8 / 2^16.
#pragma once
#include "evs_common.h"

namespace evs {

__device__ __forceinline__ long long enc_u8(double x) { return (long long)rint(((x + 1.0) / 2.0) * 254.0); }

__device__ __forceinline__ long long enc_u16(double value) {
    if (value < -0.65) {
        long long leftover = (long long)(-100.0 * (0.65 + value));
        if (leftover % 2 == 0) leftover += 1;
        return 65000 + leftover;
    } else if (value > 0.65) {
        long long leftover = (long long)(100.0 * (value - 0.65));
        if (leftover % 2 == 1) leftover -= 1;
        return 65000 + leftover;
    }
    return (long long)((value + 0.65) / 1.3 * 65000.0);
}

__device__ __forceinline__ int enc_u4(double v) {
    if (v == 0.0) return 7;
    if (v > 0.0) {
        if (v >= 0.8) return 0;
        if (v >= 0.6) return 1;
        if (v >= 0.4) return 2;
        if (v >= 0.25) return 3;
        if (v >= 0.015) return 4;
        if (v >= 0.00025) return 5;
        return 6;
    }
    if (v >= -0.00025) return 8;
    if (v < -1.0) return 15;
    if (v < -0.8) return 14;
    if (v < -0.6) return 13;
    if (v < -0.4) return 12;
    if (v < -0.25) return 11;
    if (v < -0.015) return 10;
    return 9;
}

}  // namespace evs
