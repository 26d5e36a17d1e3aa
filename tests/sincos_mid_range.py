"""The f32 angles at which mgym_math.h's sin / cos differed from glibc before reduce_fast fused x - n*pi/2 as glibc's FMA build
(__sinf_fma, __cosf_fma, __sincosf_fma) does: an enumeration of every finite f32 against glibc 2.35 on an x86-64 host with FMA
(tests/native/math_glibc_exhaustive.cpp) found these 17 magnitudes, each with both signs, all with 16 < |x| < 120, each 1 ulp
off.  A pole spun up after termination, or a lander that has turned more than 2.5 times, reaches them."""
import numpy as np

SIN_MAGNITUDES = ("0x1.ab6152p+5", "0x1.46b80ep+6", "0x1.46ba88p+6", "0x1.52e6cp+6", "0x1.9eb0a8p+6", "0x1.d0f4aap+6")
COS_MAGNITUDES = ("0x1.1475b6p+4", "0x1.1475b8p+4", "0x1.1475bap+4", "0x1.1475bcp+4", "0x1.78edb2p+4", "0x1.05d696p+5",
                  "0x1.d0f4aap+5", "0x1.019c5p+6", "0x1.0e1c8p+6", "0x1.8abf54p+6", "0x1.b1a47cp+6")
HEX = tuple(h for m in SIN_MAGNITUDES + COS_MAGNITUDES for h in (m, "-" + m))
ANGLES = np.array([float.fromhex(h) for h in HEX], np.float32)   # 34 values, exact in f32
assert len(ANGLES) == 34 and np.array_equal(ANGLES.astype(np.float64), [float.fromhex(h) for h in HEX])


def rotate_lander(s, i, angle):
    """Turn LunarLander env i of a state blob s ([state_cols][n], the reference's raw_* words: {x, y, angle, vx, vy, w} of the
    lander, leg 0, leg 1) rigidly about the lander's centre so that the lander's angle word becomes exactly `angle`: every
    leg's angle gets the same offset and its centre turns with it, so the revolute joints stay where they were."""
    a0 = float(s[2, i])
    d = float(angle) - a0
    c, sn = np.cos(d), np.sin(d)
    cx, cy = float(s[0, i]), float(s[1, i])
    s[2, i] = np.float32(angle)
    for base in (6, 12):
        px, py = float(s[base, i]) - cx, float(s[base + 1, i]) - cy
        s[base, i] = np.float32(cx + c * px - sn * py)
        s[base + 1, i] = np.float32(cy + sn * px + c * py)
        s[base + 2, i] = np.float32(float(s[base + 2, i]) + d)
