// lio_hostmath.hip -- the host-side scalar code of include/liogpu.h: lio_transform_update and lio_imu_deskew_info.  Plain
// fp64 C++ without a HIP call.  MO = mapOptmization.cpp, IP = imageProjection.cpp of the reference (liorf).
#include <math.h>
#include <stdint.h>

#include "../../include/liogpu.h"

// transformUpdate, MO:1867-1897: roll/pitch are slerp-blended towards the IMU
// attitude with tf (Bullet) quaternions in fp64, then clamped (MO:1892-1894,
// constraintTransformation MO:1899-1907).  tf::Quaternion::setRPY / slerp /
// tf::Matrix3x3::getRPY restated from their published formulas.
namespace {
struct Quat { double x, y, z, w; };

Quat quat_from_rpy(double roll, double pitch, double yaw)
{
    const double hy = yaw * 0.5, hp = pitch * 0.5, hr = roll * 0.5;
    const double cy = cos(hy), sy = sin(hy), cp = cos(hp), sp = sin(hp), cr = cos(hr), sr = sin(hr);
    return { sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
             cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy };
}

double quat_dot(const Quat& a, const Quat& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

Quat quat_slerp(const Quat& a, const Quat& q, double t)
{
    const double s = sqrt(quat_dot(a, a) * quat_dot(q, q));
    const double d = quat_dot(a, q);
    const double theta = ((d < 0) ? acos(-d / s) * 2.0 : acos(d / s) * 2.0) / 2.0;   // angleShortestPath / 2
    if (theta != 0.0) {
        const double inv = 1.0 / sin(theta);
        const double s0 = sin((1.0 - t) * theta), s1 = sin(t * theta);
        if (d < 0)
            return { (a.x * s0 + -q.x * s1) * inv, (a.y * s0 + -q.y * s1) * inv,
                     (a.z * s0 + -q.z * s1) * inv, (a.w * s0 + -q.w * s1) * inv };
        return { (a.x * s0 + q.x * s1) * inv, (a.y * s0 + q.y * s1) * inv,
                 (a.z * s0 + q.z * s1) * inv, (a.w * s0 + q.w * s1) * inv };
    }
    return a;
}

void quat_to_rpy(const Quat& q, double& roll, double& pitch, double& yaw)
{
    const double s = 2.0 / quat_dot(q, q);
    const double xs = q.x * s, ys = q.y * s, zs = q.z * s;
    const double wx = q.w * xs, wy = q.w * ys, wz = q.w * zs;
    const double xx = q.x * xs, xy = q.x * ys, xz = q.x * zs;
    const double yy = q.y * ys, yz = q.y * zs, zz = q.z * zs;
    const double m00 = 1.0 - (yy + zz), m10 = xy + wz, m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
    if (fabs(m20) >= 1) {
        yaw = 0;
        const double delta = atan2(m21, m22);
        pitch = (m20 < 0) ? M_PI / 2.0 : -M_PI / 2.0;
        roll = delta;
    } else {
        pitch = -asin(m20);
        const double cp = cos(pitch);
        roll = atan2(m21 / cp, m22 / cp);
        yaw = atan2(m10 / cp, m00 / cp);
    }
}

float clamp_abs(float v, float limit)
{
    if (v < -limit) v = -limit;
    if (v > limit) v = limit;
    return v;
}
}  // namespace

extern "C" void lio_transform_update(float pose[6], int32_t imu_available, int32_t imu_type,
                                     float imu_roll_init, float imu_pitch_init, float imu_rpy_weight,
                                     float rotation_tollerance, float z_tollerance)
{
    if (imu_available && imu_type) {                     // MO:1869
        if (fabsf(imu_pitch_init) < 1.4) {               // MO:1871
            const double w = imu_rpy_weight;
            double r, p, y;
            quat_to_rpy(quat_slerp(quat_from_rpy(pose[0], 0, 0), quat_from_rpy(imu_roll_init, 0, 0), w), r, p, y);
            pose[0] = (float)r;                          // MO:1879-1882
            quat_to_rpy(quat_slerp(quat_from_rpy(0, pose[1], 0), quat_from_rpy(0, imu_pitch_init, 0), w), r, p, y);
            pose[1] = (float)p;                          // MO:1885-1888
        }
    }
    pose[0] = clamp_abs(pose[0], rotation_tollerance);   // MO:1892
    pose[1] = clamp_abs(pose[1], rotation_tollerance);   // MO:1893
    pose[5] = clamp_abs(pose[5], z_tollerance);          // MO:1894
}

// imuDeskewInfo, IP:359-418: gyro integration over [timeScanCur-0.01, timeScanEnd+0.01]
extern "C" int lio_imu_deskew_info(const double* stamp, const double* gx, const double* gy, const double* gz,
                                   int32_t n_imu, double t_cur, double t_end,
                                   double* imuTime, double* imuRotX, double* imuRotY, double* imuRotZ)
{
    if (!stamp || !gx || !gy || !gz || !imuTime || !imuRotX || !imuRotY || !imuRotZ) return 0;
    int i = 0;
    while (i < n_imu && stamp[i] < t_cur - 0.01) ++i;    // IP:363-369
    if (i >= n_imu) return 0;                            // IP:371-372
    int cur = 0;
    for (; i < n_imu; ++i) {
        const double t = stamp[i];
        if (t > t_end + 0.01) break;                     // IP:387-388
        if (cur == 0) {                                  // IP:390-397
            imuRotX[0] = 0; imuRotY[0] = 0; imuRotZ[0] = 0; imuTime[0] = t;
            cur = 1;
            continue;
        }
        if (cur >= 2000) break;                          // table length, IP:62
        const double dt = t - imuTime[cur - 1];          // IP:404
        imuRotX[cur] = imuRotX[cur - 1] + gx[i] * dt;    // IP:405-407
        imuRotY[cur] = imuRotY[cur - 1] + gy[i] * dt;
        imuRotZ[cur] = imuRotZ[cur - 1] + gz[i] * dt;
        imuTime[cur] = t;
        ++cur;
    }
    return cur - 1;                                      // IP:412
}
