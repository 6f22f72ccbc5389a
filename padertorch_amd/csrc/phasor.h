// |X| and the unit phasor X / |X| of one spectrum bin (angle(0) := 0 like np.angle): shared by the fused PIT features (stft.hip) and
// the Griffin-Lim projection (griffin_lim.hip, the fused update in stft.hip).
#pragma once
#include "fft_regs.h"

namespace ptmi {

__device__ __forceinline__ void mag_phasor(cpx X, float& mag, cpx& ph) {
    const float p = X.x * X.x + X.y * X.y;
    const float r = __builtin_amdgcn_rsqf(p);            // 1/|X|; inf at 0 and for a DENORMAL p (the hardware flushes the operand)
    mag = p * r;
    ph = cpx{X.x * r, X.y * r};
    // (a NaN bin - a NaN sample in the frame - fails the comparison and stays NaN in the magnitude and in the phasor like np.abs /
    //  np.angle of the reference's features (pit/data.py:67-75), so that the loss and with it the Trainer's non-finite check see it)
    if (__builtin_expect(p < 1.1754944e-38f, 0)) {
        // zero or below the normal range (rare: a frame whose only samples meet window taps of ~1e-17 - a Blackman window's first tap
        // - gives |X|^2 ~ 1e-38; `p * rsq(p)` was inf there, round 6): the same arithmetic on 2^64 X
        const cpx Xs{X.x * 0x1p64f, X.y * 0x1p64f};
        const float ps = Xs.x * Xs.x + Xs.y * Xs.y;
        const float rs = __builtin_amdgcn_rsqf(ps);
        const bool zero = ps < 1.1754944e-38f;           // |X| < 2^-127: zero like the exact zero (angle(0) := 0)
        mag = zero ? 0.f : ps * rs * 0x1p-64f;
        ph = zero ? cpx{1.f, 0.f} : cpx{Xs.x * rs, Xs.y * rs};
    }
}

}  // namespace ptmi
