// The wave-level end of one ball query, shared by ballfeat.hip (a cloud about its own points) and cloud_distance.hip (external queries):
// the butterfly that merges the lanes' sums, ball_point.h's finish, and the stores of the outputs both kernels have.
#pragma once
#include "common.h"
#include "ball_point.h"

namespace im {
namespace {

static_assert(BALL_SUMS <= IM_WAVE, "the sums are stored by the first lanes of a wave");

// S: this lane's sums in, the ball's sums out (in every lane); eig and e3 out for what the caller derives from them. Every output pointer
// may be null; all are addressed by the query's index qi.
__device__ __forceinline__ void ball_wave_finish(BallSums& S, int lane, long long qi, double hh, int steps, int* count, long long* sums,
                                                 double* eig_out, double* normal, int* steps_out, double (&eig)[3], double (&e3)[3]) {
    // integer sums: any order gives the same bits, so the butterfly leaves the ball's sums in every lane
#pragma unroll
    for (int k = 0; k < BALL_SUMS; ++k)
#pragma unroll
        for (int o = IM_WAVE / 2; o > 0; o >>= 1) S.s[k] += __shfl_xor(S.s[k], o);
    ball_finish(S, hh, eig, e3);
    if (lane == 0) {
        if (count) count[qi] = (int)S.s[0];
        if (steps_out) steps_out[qi] = steps;
    }
    if (sums) {
        long long v = 0;
#pragma unroll
        for (int k = 0; k < BALL_SUMS; ++k) v = lane == k ? S.s[k] : v;
        if (lane < BALL_SUMS) sums[qi * BALL_SUMS + lane] = v;
    }
    if (lane < 3) {
        if (eig_out) eig_out[3 * qi + lane] = lane == 0 ? eig[0] : (lane == 1 ? eig[1] : eig[2]);
        if (normal) normal[3 * qi + lane] = lane == 0 ? e3[0] : (lane == 1 ? e3[1] : e3[2]);
    }
}

}  // namespace
}  // namespace im
