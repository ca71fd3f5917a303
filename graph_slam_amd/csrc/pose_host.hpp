// Host-side pose arithmetic shared by the map calls that turn a pose7 (t, q_xyzw) into the 12 numbers rt = R row-major, then t, which
// their kernels use (map fusion, map rendering).  include/fgo.h states the expressions; every product, quotient and sum is rounded on
// its own (contraction is off in every function here), so that the numpy restatements of the tests reproduce rt bit for bit.
// quat_ok, the validator that goes with them, is in batch_call.hpp, which includes this file, as is poses_rt: rt of all poses of a call.
#pragma once
#include <cmath>
#include <cstring>

namespace fgo {

// R of a quaternion that quat_ok accepted: normalised, then the nine expressions of the header, every operation rounded on its own
inline void quat_matrix(const double *q, double R[9]) {
#pragma clang fp contract(off)
  const double n = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const double x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w); R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w); R[7] = 2.0 * (y * z + x * w); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// rt = R row-major, then t, of the pose (times the extrinsic)
inline void pose_rt(const double *pose7, const double *ext7, double rt[12]) {
#pragma clang fp contract(off)
  double Rw[9];
  quat_matrix(pose7 + 3, Rw);
  if (!ext7) {
    std::memcpy(rt, Rw, sizeof Rw);
    for (int k = 0; k < 3; ++k) rt[9 + k] = pose7[k];
    return;
  }
  double Re[9];
  quat_matrix(ext7 + 3, Re);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) rt[3 * i + j] = (Rw[3 * i] * Re[j] + Rw[3 * i + 1] * Re[3 + j]) + Rw[3 * i + 2] * Re[6 + j];
    rt[9 + i] = ((Rw[3 * i] * ext7[0] + Rw[3 * i + 1] * ext7[1]) + Rw[3 * i + 2] * ext7[2]) + pose7[i];
  }
}

// rt = rt1 with the pose off7 composed on the right: R = R1 Ro, t = R1 to + t1.  rt may not alias rt1.
inline void rt_compose(const double rt1[12], const double *off7, double rt[12]) {
#pragma clang fp contract(off)
  double Ro[9];
  quat_matrix(off7 + 3, Ro);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) rt[3 * i + j] = (rt1[3 * i] * Ro[j] + rt1[3 * i + 1] * Ro[3 + j]) + rt1[3 * i + 2] * Ro[6 + j];
    rt[9 + i] = ((rt1[3 * i] * off7[0] + rt1[3 * i + 1] * off7[1]) + rt1[3 * i + 2] * off7[2]) + rt1[9 + i];
  }
}

}  // namespace fgo
