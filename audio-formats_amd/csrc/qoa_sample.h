// qoa_sample.h -- the int16 sample the QOA encoder sees for a float or double input x, as include/afg.h defines it
// (afg_qoa_encode_hip): QOAEncoder.writeSamples (qoa.d:632-636) as a release build of the reference executes it on
// x86-64.  There cast(int) of a double is cvttsd2si -- truncation toward zero, INT_MIN ("integer indefinite") for NaN
// and for anything outside the int range -- and cast(short) keeps the low 16 bits.  A plain (int) of such a value is
// undefined behaviour in C++ and the device's v_cvt_i32_f64 saturates instead, so the range is tested first; the kernel
// (csrc/qoa_encode.hip) and the write stream (host/afg_write_stream.cpp) both convert through this one function.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AFG_QOA_HD __host__ __device__ inline
#else
#define AFG_QOA_HD inline
#endif

AFG_QOA_HD int16_t afg_qoa_sample(double x)
{
    const double v = 32768.5 + x * 32767.0;
    const int32_t t = (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN;     // NaN fails both tests
    return (int16_t)(uint16_t)((uint32_t)t - 32768u);
}
