// The activation codes of ptmi_je_conv_* and their device functions, shared by csrc/je_conv.hip and csrc/je_conv2d.hip.
#pragma once
#include "reduce.h"

namespace ptmi {

enum { kActIdentity = 0, kActRelu = 1, kActLeaky = 2, kActElu = 3, kActTanh = 4, kActSigmoid = 5, kActPrelu = 6 };

__device__ __forceinline__ long long jc_len(const void* lengths, int is64, long long b, long long T) {
    if (!lengths) return T;
    const long long n = is64 ? static_cast<const long long*>(lengths)[b] : (long long)static_cast<const int*>(lengths)[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

__device__ __forceinline__ float jc_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

__device__ __forceinline__ float jc_act(float v, int act, float p) {
    switch (act) {
        case kActRelu: return v < 0.f ? 0.f : v;
        case kActLeaky:
        case kActPrelu: return v < 0.f ? p * v : v;
        case kActElu: return v > 0.f ? v : p * expm1f(v);
        case kActTanh: return tanhf(v);
        case kActSigmoid: return jc_sigmoid(v);
        default: return v;
    }
}

// d act / d v at the pre-activation v
__device__ __forceinline__ float jc_dact(float v, int act, float p) {
    switch (act) {
        case kActRelu: return v > 0.f ? 1.f : 0.f;
        case kActLeaky:
        case kActPrelu: return v > 0.f ? 1.f : p;
        case kActElu: return v > 0.f ? 1.f : p * expf(v);
        case kActTanh: {
            const float t = tanhf(v);
            return 1.f - t * t;
        }
        case kActSigmoid: {
            const float s = jc_sigmoid(v);
            return s * (1.f - s);
        }
        default: return 1.f;
    }
}

}  // namespace ptmi
