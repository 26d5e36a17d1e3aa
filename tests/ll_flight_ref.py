"""Float64 reference of one airborne LunarLander step, from the definitions alone: plain numpy, vectorised over cases, nothing from
the engine or the oracle.  Three bodies, two revolute joints with limit and motor (Box2D's sequential-impulse solver as its manual
and b2_revolute_joint / b2_island define it), gravity, wind, the two engine impulses of lunar_lander.rs:962-1048, then observation
and reward (:1095-1156).  No contacts: the cases (tests/ll_flight_cases.py) stay above every terrain vertex.

Constants are the reference's f32 constants, combined as src/box_2d/lunar_lander.rs combines them; everything after is float64.
Masses, inertias about the centroid and local centres come from ll_geom_ref.polygon_mass.

State, per body, in the state blob's convention: body-origin position p, angle a, centre-of-mass velocity v, angular velocity w.
Each joint carries its accumulated impulses (P, motor, lower, upper), 0 in a new world.

Bounds.  MEASURED_* is the worst absolute deviation of the CPU oracle from this reference, per group, over the seeded cases and
the non-clamp hand-built classes of ll_flight_cases.py (12 steps, wind off and wind on at the default parameters), and over the
clamp classes (150 m/s, 600 rad/s relative, 100 rad/s spin) on their own; BOUND_* = 4 x measured, the factor covering the other
parameter sets and the f32 paths that differ by rounding only.  Reproduce with
    python tests/ll_flight_cases.py --measure
The groups: lander position / angle, lander velocities, leg position / angle, leg velocities, observation, reward, and the
dispersion differential (test (b) of tests/test_ll_flight_oracle.py; DIFF over the same two sets of classes).  The oracle is built
with -ffp-contract=off, so only the host libm's last bit of sinf / cosf / tanhf can move the figures, far below them.  Limits that are no
measurements: a BOUND above 5e-4 for the lander groups, 5e-3 for the leg groups or 5e-5 for the differential would mean the
reference or the protocol is wrong (asserted below; 4 x MEASURED_DIFF is 5.5e-5 and is held to the 5e-5).  What the deviations are
made of: the median over cases is a few f32 spacings; the tail comes from cases whose position sweeps converge slowly (a leg's
origin starts up to 0.05 from its anchor, and 60 sweeps at a mass ratio of 68 do not always close that), where f32 rounding is
amplified, and from "solved" decisions that fall within rounding of the slop, where one sweep more or less moves a leg by 1.7e-4.

Two places where the step is not what the issue that asked for this file said.  The joints are swept in the order leg 1, leg 0 (see
FlightRef.ORDER), not 0, 1: with the other order the oracle is 1e-3 away after one step, the clamp classes by more than 1.  And the
differential's reference starts from reset()'s own impulses, not from zero (ll_flight_cases.reference_after_reset)."""
import numpy as np

import ll_geom_ref as G

GROUPS = ("lander_pose", "lander_vel", "leg_pose", "leg_vel", "obs", "reward")
MEASURED = dict(lander_pose=4.15e-05, lander_vel=1.05e-04, leg_pose=1.69e-04, leg_vel=1.19e-03, obs=4.21e-05, reward=2.58e-03)
MEASURED_CLAMP = dict(lander_pose=2.68e-04, lander_vel=9.36e-04, leg_pose=1.61e-04, leg_vel=2.27e-03, obs=3.74e-04, reward=5.20e-03)
MEASURED_DIFF = 1.38e-05
MEASURED_DIFF_CLAMP = 7.90e-05
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
BOUND_CLAMP = {k: 4.0 * v for k, v in MEASURED_CLAMP.items()}
BOUND_DIFF, BOUND_DIFF_CLAMP = min(4.0 * MEASURED_DIFF, 5e-5), 4.0 * MEASURED_DIFF_CLAMP   # (4 x measured is 5.5e-5: held to the limit)
assert max(BOUND["lander_pose"], BOUND["lander_vel"]) <= 5e-4 and max(BOUND["leg_pose"], BOUND["leg_vel"]) <= 5e-3 and BOUND_DIFF <= 5e-5

f32 = np.float32


def _d(x):
    return float(f32(x))


# lunar_lander.rs:31-58
FPS = f32(50.0)                                   # :31
SCALE = f32(30.0)                                 # :32
MAIN_ENGINE_POWER = _d(13.0)                      # :34
SIDE_ENGINE_POWER = _d(0.6)                       # :35
LEG_AWAY, LEG_DOWN = f32(20.0), f32(18.0)         # :47-48
LEG_SPRING_TORQUE = _d(40.0)                      # :51
SIDE_ENGINE_HEIGHT = f32(14.0)                    # :53
SIDE_ENGINE_AWAY = f32(12.0)                      # :54
MAIN_ENGINE_Y_LOCATION = f32(4.0)                 # :55
VIEWPORT_W, VIEWPORT_H = f32(600.0), f32(400.0)   # :57-58
PI32 = f32(np.pi)                                 # std::f32::consts::PI, :943

H = _d(f32(1.0) / FPS)                            # :1066  world.step(1.0 / FPS, 6 * 30, 2 * 30)
VEL_ITERS, POS_ITERS = 6 * 30, 2 * 30
MAIN_Y = _d(MAIN_ENGINE_Y_LOCATION / SCALE)       # :986
W2 = _d(VIEWPORT_W / SCALE / f32(2.0))            # :1113
H2 = _d(VIEWPORT_H / SCALE / f32(2.0))            # :1114
HELIPAD_LEGS = _d(VIEWPORT_H / SCALE / f32(4.0) + LEG_DOWN / SCALE)   # :1287 helipad_y = h / 4, :1114
WIND_A, WIND_B = f32(0.02), PI32 * f32(0.01)      # :942-943

# joints, :887-902: leg 0 is i = -1
SIGN = (-1.0, 1.0)
ANCHOR_B = [np.array([_d(f32(i) * LEG_AWAY / SCALE), _d(LEG_DOWN / SCALE)]) for i in SIGN]   # :891
LOWER = (_d(f32(0.9) - f32(0.5)), _d(f32(-0.9)))              # :897, :900
UPPER = (_d(f32(0.9)), _d(f32(-0.9) + f32(0.5)))              # :898, :901
MOTOR_SPEED = (_d(f32(0.3) * f32(-1.0)), _d(f32(0.3)))        # :895

# Box2D (b2_common.h)
LINEAR_SLOP = 0.005
ANGULAR_SLOP = 2.0 / 180.0 * np.pi
MAX_ANGULAR_CORRECTION = 8.0 / 180.0 * np.pi
MAX_TRANSLATION = 2.0
MAX_ROTATION = 0.5 * np.pi

HULL = [G.shape(0), G.shape(1)]
_MASS = [G.polygon_mass(HULL[0], 5.0), G.polygon_mass(HULL[1], 1.0)]   # densities :836, :879
BODY_SHAPE = (0, 1, 1)
MASS = np.array([_MASS[s][0] for s in BODY_SHAPE])
LC = np.array([_MASS[s][1] for s in BODY_SHAPE])
INERTIA = np.array([_MASS[s][2] for s in BODY_SHAPE])
INV_M, INV_I = 1.0 / MASS, 1.0 / INERTIA

FLAGS = ("motor_clamp", "lower_limit", "upper_limit", "position_correction", "angular_clamp", "translation_clamp",
         "rotation_clamp")


def rot(a, x):
    c, s = np.cos(a), np.sin(a)
    return np.stack([c * x[..., 0] - s * x[..., 1], s * x[..., 0] + c * x[..., 1]], -1)


def cross(u, v):
    return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]


def cross_sv(s, v):
    """s x v for a scalar s: (-s v.y, s v.x)"""
    return np.stack([-s * v[..., 1], s * v[..., 0]], -1)


def _k_matrix(rA, rB, b):
    """K of the point constraint between the lander and body b, as (k11, k12, k22)"""
    m = INV_M[0] + INV_M[b]
    k11 = m + INV_I[0] * rA[:, 1] ** 2 + INV_I[b] * rB[:, 1] ** 2
    k12 = -INV_I[0] * rA[:, 0] * rA[:, 1] - INV_I[b] * rB[:, 0] * rB[:, 1]
    k22 = m + INV_I[0] * rA[:, 0] ** 2 + INV_I[b] * rB[:, 0] ** 2
    return k11, k12, k22


def _k_solve(K, b):
    k11, k12, k22 = K
    det = k11 * k22 - k12 * k12
    return np.stack([(k22 * b[:, 0] - k12 * b[:, 1]) / det, (k11 * b[:, 1] - k12 * b[:, 0]) / det], -1)


class FlightRef:
    """n airborne environments.  blob: [>= 18, n] words of the state blob (x y angle vx vy w of lander, leg 0, leg 1)."""

    # b2World::Solve builds the island depth-first from the head of the body list, the body created last (leg 1), and every
    # body's joint list has its newest joint first: the island's joints are [joint of leg 1, joint of leg 0].
    ORDER = (1, 0)

    def __init__(self, blob, gravity=-10.0, enable_wind=False, wind_power=15.0, turbulence_power=1.5, deterministic=True,
                 wind_idx=0, torque_idx=0):
        s = np.asarray(blob, np.float32)[:18].astype(np.float64).reshape(3, 6, -1)
        self.n = s.shape[2]
        self.p = np.ascontiguousarray(s[:, 0:2].transpose(2, 0, 1))    # [n, 3, 2]
        self.a = np.ascontiguousarray(s[:, 2].T)                       # [n, 3]
        self.v = np.ascontiguousarray(s[:, 3:5].transpose(2, 0, 1))
        self.w = np.ascontiguousarray(s[:, 5].T)
        self.gravity, self.enable_wind = _d(gravity), bool(enable_wind)
        self.wind_power, self.turbulence_power = _d(wind_power), _d(turbulence_power)
        self.deterministic = deterministic
        self.wind_idx = np.broadcast_to(np.asarray(wind_idx, np.int64), (self.n,)).copy()
        self.torque_idx = np.broadcast_to(np.asarray(torque_idx, np.int64), (self.n,)).copy()
        self.P = np.zeros((self.n, 2, 2))
        self.motor, self.lower, self.upper = np.zeros((self.n, 2)), np.zeros((self.n, 2)), np.zeros((self.n, 2))
        self.dt_ratio = 0.0                      # a new world: inv_dt0 = 0
        self.prev_shaping = np.full(self.n, np.nan)
        self.flags = {k: np.zeros(self.n, bool) for k in FLAGS}
        self.lowest_y = self.lowest_vertex()

    def set_words(self, blob):
        """Testable::set_state (:1444-1554): poses and velocities only; the joints keep their accumulated impulses"""
        s = np.asarray(blob, np.float32)[:18].astype(np.float64).reshape(3, 6, -1)
        self.p[:], self.a[:] = s[:, 0:2].transpose(2, 0, 1), s[:, 2].T
        self.v[:], self.w[:] = s[:, 3:5].transpose(2, 0, 1), s[:, 5].T

    def words(self):
        """the 18 pose / velocity words, [18, n] float64"""
        return np.concatenate([np.stack([self.p[:, b, 0], self.p[:, b, 1], self.a[:, b], self.v[:, b, 0], self.v[:, b, 1],
                                         self.w[:, b]]) for b in range(3)])

    def lowest_vertex(self):
        return np.min([G.world(HULL[BODY_SHAPE[b]], self.p[:, b], self.a[:, b])[..., 1].min(-1) for b in range(3)], 0)

    @staticmethod
    def _gust(k):
        """tanh(sin(0.02 k) + sin(0.01 pi k)) with the f32 products of :942-943 as arguments"""
        kf = k.astype(np.float32)
        return np.tanh(np.sin((WIND_A * kf).astype(np.float64)) + np.sin((WIND_B * kf).astype(np.float64)))

    def step(self, action, disp=None, push=None, exit_bias=0):
        """-> obs [8, n], reward [n], done [n]; self.flags and self.lowest_y describe the step.  push [n, 2]: a force on the lander's
        centre for this step (reset()'s apply_force_to_center, :845-849).  exit_bias -1 / +1: the position sweeps' "solved" test with
        both slops moved down / up by G.fp_slack of the case's largest coordinate and angle, i.e. the other outcome of a decision
        that f32 arithmetic can take either way; self.exit_margin says how close the decisions came."""
        n = self.n
        action = np.asarray(action).astype(np.int64)
        p, a, v, w = self.p, self.a, self.v, self.w
        c = p + rot(a, LC[None])                          # centres of mass
        force, torque = np.zeros((n, 2)) if push is None else np.array(push, np.float64), np.zeros(n)
        if self.enable_wind:                                         # :927-959; no leg touches anything here
            force[:, 0] += self._gust(self.wind_idx) * self.wind_power
            torque = self._gust(self.torque_idx) * self.turbulence_power
            self.wind_idx += 1
            self.torque_idx += 1

        # engines, :962-1048
        tip = np.stack([np.sin(a[:, 0]), np.cos(a[:, 0])], -1)
        side = np.stack([-tip[:, 1], tip[:, 0]], -1)
        if self.deterministic or disp is None:
            d = np.zeros((2, n))
        else:
            d = np.asarray(disp, np.float32).astype(np.float64) / float(SCALE)      # :973-974
        main, fire_side = action == 2, (action == 1) | (action == 3)
        direction = (action - 2).astype(np.float64)                  # :1024

        def impulse(J, r, on):
            J = np.where(on[:, None], J, 0.0)
            v[:, 0] += INV_M[0] * J
            w[:, 0] += INV_I[0] * cross(r - c[:, 0], J)

        mo = MAIN_Y + 2.0 * d[0]                                     # :986-989
        o = np.stack([tip[:, 0] * mo + side[:, 0] * d[1], -tip[:, 1] * mo - side[:, 1] * d[1]], -1)
        impulse(-o * MAIN_ENGINE_POWER, p[:, 0] + o, main)           # :991-1003
        so = 3.0 * d[1] + direction * float(SIDE_ENGINE_AWAY) / float(SCALE)         # :1028-1031
        o = np.stack([tip[:, 0] * d[0] + side[:, 0] * so, -tip[:, 1] * d[0] - side[:, 1] * so], -1)
        at = p[:, 0] + o + np.stack([-tip[:, 0] * 17.0 / float(SCALE), tip[:, 1] * float(SIDE_ENGINE_HEIGHT) / float(SCALE)], -1)
        impulse(-o * SIDE_ENGINE_POWER, at, fire_side)               # :1033-1048

        # b2Island::Solve: integrate velocities (no damping), solve, integrate positions, correct positions
        v[:, :, 1] += H * self.gravity
        v[:, 0] += H * INV_M[0] * force
        w[:, 0] += H * INV_I[0] * torque

        rA = [rot(a[:, 0], -LC[0]) for _ in range(2)]
        rB = [rot(a[:, 1 + j], ANCHOR_B[j] - LC[1 + j]) for j in range(2)]
        K = [_k_matrix(rA[j], rB[j], 1 + j) for j in range(2)]
        axial = [1.0 / (INV_I[0] + INV_I[1 + j]) for j in range(2)]
        angle = [a[:, 1 + j] - a[:, 0] for j in range(2)]
        vl, wl = v[:, 0].copy(), w[:, 0].copy()
        vg, wg = [v[:, 1 + j].copy() for j in range(2)], [w[:, 1 + j].copy() for j in range(2)]
        for j in range(2):                                           # warm start
            b = 1 + j
            for x in (self.P, self.motor, self.lower, self.upper):
                x[:, j] *= self.dt_ratio
            ax = self.motor[:, j] + self.lower[:, j] - self.upper[:, j]
            Pj = self.P[:, j]
            vl -= INV_M[0] * Pj
            wl -= INV_I[0] * (cross(rA[j], Pj) + ax)
            vg[j] += INV_M[b] * Pj
            wg[j] += INV_I[b] * (cross(rB[j], Pj) + ax)
        max_motor = LEG_SPRING_TORQUE * H
        for _ in range(VEL_ITERS):
            for j in self.ORDER:
                b = 1 + j
                iA, iB = INV_I[0], INV_I[b]
                # motor
                imp = -axial[j] * (wg[j] - wl - MOTOR_SPEED[j])
                new = np.clip(self.motor[:, j] + imp, -max_motor, max_motor)
                imp = new - self.motor[:, j]
                self.motor[:, j] = new
                wl -= iA * imp
                wg[j] += iB * imp
                # lower limit
                C = angle[j] - LOWER[j]
                imp = -axial[j] * (wg[j] - wl + np.maximum(C, 0.0) / H)
                new = np.maximum(self.lower[:, j] + imp, 0.0)
                imp = new - self.lower[:, j]
                self.lower[:, j] = new
                wl -= iA * imp
                wg[j] += iB * imp
                # upper limit
                C = UPPER[j] - angle[j]
                imp = -axial[j] * (wl - wg[j] + np.maximum(C, 0.0) / H)
                new = np.maximum(self.upper[:, j] + imp, 0.0)
                imp = new - self.upper[:, j]
                self.upper[:, j] = new
                wl += iA * imp
                wg[j] -= iB * imp
                # point
                cdot = vg[j] + cross_sv(wg[j], rB[j]) - vl - cross_sv(wl, rA[j])
                imp = _k_solve(K[j], -cdot)
                self.P[:, j] += imp
                vl -= INV_M[0] * imp
                wl -= iA * cross(rA[j], imp)
                vg[j] += INV_M[b] * imp
                wg[j] += iB * cross(rB[j], imp)
        self.dt_ratio = 1.0
        v[:, 0], w[:, 0] = vl, wl
        for j in range(2):
            v[:, 1 + j], w[:, 1 + j] = vg[j], wg[j]
        fl = self.flags = {k: np.zeros(n, bool) for k in FLAGS}
        fl["motor_clamp"] = (np.abs(self.motor) >= max_motor).any(1)
        fl["lower_limit"] = (self.lower > 0.0).any(1)
        fl["upper_limit"] = (self.upper > 0.0).any(1)

        # integrate positions with Box2D's clamps
        tr = H * v
        ln = np.sqrt((tr * tr).sum(-1))
        big = ln > MAX_TRANSLATION
        v *= np.where(big, MAX_TRANSLATION / np.where(big, ln, 1.0), 1.0)[..., None]
        rt = np.abs(H * w)
        bigr = rt > MAX_ROTATION
        w *= np.where(bigr, MAX_ROTATION / np.where(bigr, rt, 1.0), 1.0)
        fl["translation_clamp"], fl["rotation_clamp"] = big.any(1), bigr.any(1)
        c = c + H * v
        a += H * w

        # position sweeps; every environment leaves on its own
        active = np.ones(n, bool)
        lin_slop = LINEAR_SLOP + exit_bias * G.fp_slack(np.abs(c).max((1, 2)))
        ang_slop = ANGULAR_SLOP + exit_bias * G.fp_slack(np.maximum(np.abs(a).max(1), 1.0))
        self.pos_sweeps, self.exit_margin = np.zeros(n, int), np.full(n, np.inf)
        for _ in range(POS_ITERS):
            self.pos_sweeps += active
            ok = np.ones(n, bool)
            for j in self.ORDER:
                b = 1 + j
                ang = a[:, b] - a[:, 0]
                raw = np.where(ang <= LOWER[j], ang - LOWER[j] + ANGULAR_SLOP, np.where(ang >= UPPER[j], ang - UPPER[j] - ANGULAR_SLOP, 0.0))
                C = np.where(ang <= LOWER[j], np.clip(raw, -MAX_ANGULAR_CORRECTION, 0.0),
                             np.where(ang >= UPPER[j], np.clip(raw, 0.0, MAX_ANGULAR_CORRECTION), 0.0))
                fl["position_correction"] |= active & (C != 0.0)
                fl["angular_clamp"] |= active & (np.abs(raw) > MAX_ANGULAR_CORRECTION)
                li = np.where(active, -axial[j] * C, 0.0)
                a[:, 0] -= INV_I[0] * li
                a[:, b] += INV_I[b] * li
                ok &= np.abs(C) <= ang_slop
                self.exit_margin = np.where(active, np.minimum(self.exit_margin, np.abs(np.abs(C) - ANGULAR_SLOP)), self.exit_margin)
                ra = rot(a[:, 0], -LC[0])
                rb = rot(a[:, b], ANCHOR_B[j] - LC[b])
                Cp = c[:, b] + rb - c[:, 0] - ra
                ok &= np.sqrt((Cp * Cp).sum(-1)) <= lin_slop
                self.exit_margin = np.where(active, np.minimum(self.exit_margin, np.abs(np.sqrt((Cp * Cp).sum(-1)) - LINEAR_SLOP)), self.exit_margin)
                imp = np.where(active[:, None], -_k_solve(_k_matrix(ra, rb, b), Cp), 0.0)
                c[:, 0] -= INV_M[0] * imp
                a[:, 0] -= INV_I[0] * cross(ra, imp)
                c[:, b] += INV_M[b] * imp
                a[:, b] += INV_I[b] * cross(rb, imp)
            active &= ~ok
            if not active.any():
                break
        self.p[:] = c - rot(a, LC[None])
        self.lowest_y = self.lowest_vertex()
        return self._observe(main, fire_side)

    def _observe(self, main, fire_side):
        """:1095-1156; the legs touch nothing"""
        n = self.n
        x, y = self.p[:, 0, 0], self.p[:, 0, 1]
        obs = np.stack([(x - W2) / W2, (y - HELIPAD_LEGS) / H2, self.v[:, 0, 0] * W2 / float(FPS), self.v[:, 0, 1] * H2 / float(FPS),
                        self.a[:, 0], 20.0 * self.w[:, 0] / float(FPS), np.zeros(n), np.zeros(n)])
        shaping = -100.0 * np.hypot(obs[0], obs[1]) - 100.0 * np.hypot(obs[2], obs[3]) - 100.0 * np.abs(obs[4])
        reward = np.where(np.isnan(self.prev_shaping), 0.0, shaping - np.where(np.isnan(self.prev_shaping), 0.0, self.prev_shaping))
        self.prev_shaping = shaping
        reward = reward - np.where(main, _d(0.30), 0.0) - np.where(fire_side, _d(0.03), 0.0)   # :1138-1139
        done = np.abs(obs[0]) >= 1.0                                                           # :1150
        reward = np.where(done, -100.0, reward)
        return obs, reward, done
