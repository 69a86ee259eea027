// msckf_correct.h -- the state correction of an EKF update (msckf.py:566-595) as
// device code shared by its two callers: k_correct (the feature update,
// msckf_kernels.hip) and k_zupt_gain (the zero-velocity update, msckf_zupt.hip).
#pragma once
#include "msckf_common.h"

namespace msckf {

// Filter b's IMU record and its nc cam states take the correction dxk (fp64,
// error-state order of msckf_hip.h, 21 + 6 nc entries; global or LDS).  Thread 0
// of the workgroup corrects the IMU record, the cams are dealt over the threads.
template <typename T>
__device__ __forceinline__ void correct_state(const DevState<T>& st, int b, const KT* dxk) {
    T dxs[21];
    for (int i = 0; i < 21; ++i) dxs[i] = (T)dxk[i];
    const T* dx = dxs;
    T* imu = st.imu + (size_t)b * IMU_STRIDE;
    const int nc = st.ncams[b];
    const int tid = threadIdx.x;
    if (tid == 0) {
        T dq[4], q[4];
        small_angle_quat(dx, dq);
        quat_mul(dq, imu + I_Q, q);
        for (int i = 0; i < 4; ++i) imu[I_Q + i] = q[i];
        for (int i = 0; i < 3; ++i) {
            imu[I_BG + i] += dx[3 + i];
            imu[I_V + i] += dx[6 + i];
            imu[I_BA + i] += dx[9 + i];
            imu[I_P + i] += dx[12 + i];
        }
        T dqe[4], Re[9], Rn[9];
        small_angle_quat(dx + 15, dqe);
        quat_to_rot(dqe, Re);
        mat3_mul(Re, imu + I_RIC, Rn);
        for (int e = 0; e < 9; ++e) imu[I_RIC + e] = Rn[e];
        for (int i = 0; i < 3; ++i) imu[I_TCI + i] += dx[18 + i];
    }
    T* cams = st.cams + (size_t)b * st.Nmax * CAM_STRIDE;
    for (int c = tid; c < nc; c += blockDim.x) {
        T d[6];
        for (int i = 0; i < 6; ++i) d[i] = (T)dxk[21 + 6 * c + i];
        T dq[4], q[4];
        small_angle_quat(d, dq);
        quat_mul(dq, cams + (size_t)c * CAM_STRIDE + C_Q, q);
        for (int i = 0; i < 4; ++i) cams[(size_t)c * CAM_STRIDE + C_Q + i] = q[i];
        for (int i = 0; i < 3; ++i) cams[(size_t)c * CAM_STRIDE + C_P + i] += d[3 + i];
    }
}

}  // namespace msckf
