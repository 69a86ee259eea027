"""Filter configuration for the MI355X MSCKF update path.

Mirrors the filter-relevant fields of the reference ConfigEuRoC /
OptimizationConfigEuRoC (MSCKF/config.py:5-124).  Front-end fields (FAST,
KLT, grid) are out of scope and not carried.  Values are the reference's
defaults.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# chi2.ppf(0.05, dof) for dof = 1..99, exactly as the reference builds it
# (MSCKF/msckf.py:121-123 -- note the 5 % LOWER quantile, quirk Q6).  Generated
# once with scipy 1.15.3 and frozen here so that no scipy is needed at run time.
CHI2_05 = (
    0.003932140000019522, 0.10258658877510106, 0.35184631774927144,
    0.7107230213973239, 1.1454762260617692, 1.6353828943279067,
    2.167349909298057, 2.732636793499662, 3.325112843066815,
    3.9402991361190605, 4.574813079322224, 5.226029488392639,
    5.8918643377098485, 6.57063138378934, 7.2609439276700325,
    7.9616455723785515, 8.671760204670077, 9.390455080688984,
    10.117013063859044, 10.85081139418259, 11.591305208820733,
    12.338014578790643, 13.090514188172804, 13.848425027170224,
    14.61140763948331, 15.379156583261723, 16.151395849664098,
    16.927875044422496, 17.70836618282458, 18.49266098195347,
    19.280568559129293, 20.071913464548288, 20.86653399071479,
    21.664280712551975, 22.465015220882684, 23.268609018893773,
    24.07494255667991, 24.883904383335626, 25.695390399574777,
    26.50930319669311, 27.32555146999419, 28.144049496682623,
    28.964716669775694, 29.787477080861958, 30.612259145595477,
    31.43899526669704, 32.26762152997339, 33.09807742948629,
    33.93030561852784, 34.76425168350175, 35.5998639381883,
    36.437093236191636, 37.275892799644296, 38.1162180624794,
    38.95802652678509, 39.80127763093126, 40.64593262831063,
    41.491954475668955, 42.33930773011346, 43.187958453989765,
    44.03787412690472, 44.88902356425022, 45.741376841650336,
    46.594905224813964, 47.44958110432793, 48.30537793497176,
    49.16227017917681, 50.020233254289266, 50.879243483328636,
    51.73927804896291, 52.60031495044724, 53.462332963296205,
    54.325311601480685, 55.1892310819587, 56.05407229136661,
    56.91981675471199, 57.78644660592318, 58.65394456012262,
    59.52229388750226, 60.391478388689464, 61.261482371500676,
    62.13229062898852, 63.003888418695496, 63.87626144303417,
    64.74939583071999, 65.62327811918864, 66.49789523793463,
    67.37323449271317, 68.24928355055083, 69.12603042551552,
    70.00346346519876, 70.88157133786743, 71.76034302024499,
    72.63976778588469, 73.5198351941001, 74.40053507942093,
    75.28185754154367, 76.16379293574907, 77.04633186376029,
)


def chi2_threshold(dof: int) -> float:
    """Reference chi_squared_test_table[dof] (msckf.py:611).  The table has
    keys 1..99; any other dof raises KeyError like the reference dict."""
    if dof < 1 or dof > 99:
        raise KeyError(dof)
    return CHI2_05[dof - 1]


# chi2.ppf(0.95, dof) for dof = 1..12: the UPPER 0.95 quantiles, the gate of the
# aiding fixes (include/msckf_aid.h).  chi2_threshold is the reference's lower
# 0.05 tail (quirk Q6) and would reject 95 % of good fixes.
CHI2_95 = (
    3.841458820694124, 5.991464547107979, 7.814727903251179,
    9.487729036781154, 11.070497693516351, 12.591587243743977,
    14.067140449340169, 15.50731305586545, 16.918977604620448,
    18.307038053275146, 19.67513757268249, 21.02606981748307,
)


@dataclass
class OptimizationConfig:
    """Reference OptimizationConfigEuRoC (config.py:5-15)."""
    translation_threshold: float = -1.0
    huber_epsilon: float = 0.01
    estimation_precision: float = 5e-7
    initial_damping: float = 1e-3
    outer_loop_max_iteration: int = 5
    inner_loop_max_iteration: int = 5


def _default_T_imu_cam0():
    return np.array([
        [0.014865542981794, 0.999557249008346, -0.025774436697440, 0.065222909535531],
        [-0.999880929698575, 0.014967213324719, 0.003756188357967, -0.020706385492719],
        [0.004140296794224, 0.025715529947966, 0.999660727177902, -0.008054602460030],
        [0, 0, 0, 1.000000000000000]])


def _default_T_cn_cnm1():
    return np.array([
        [0.999997256477881, 0.002312067192424, 0.000376008102415, -0.110073808127187],
        [-0.002317135723281, 0.999898048506644, 0.014089835846648, 0.000399121547014],
        [-0.000343393120525, -0.014090668452714, 0.999900662637729, -0.000853702503357],
        [0, 0, 0, 1.000000000000000]])


_ZUPT_ROWS = {"vel": 1, "gyro": 2, "acc": 4}   # MSCKF_ZUPT_VEL / GYRO / ACC (include/msckf_zupt.h)


_CUE_MODES = ("veto", "either")       # MSCKF_CUE_MODE_VETO / EITHER (include/msckf_standstill.h)
_CUE_UNKNOWNS = ("imu", "reject")     # MSCKF_CUE_UNKNOWN_IMU / REJECT


@dataclass
class VisionCue:
    """The vision standstill cue of the zero-velocity update
    (include/msckf_standstill.h): the ``quantile`` of the squared frame-to-frame
    pixel displacement of the front-end's tracks says STILL when it is at most
    ``max_px``^2, provided at least ``min_tracks`` tracks stand behind it.

    ``mode``: "veto" -- the update needs the IMU gate AND a still image;
    "either" -- a still image applies it even where the speed or chi^2 gate
    refuses.  ``unknown``: what a frame without a usable cue does, "imu" (the
    IMU gate alone decides, as without a cue) or "reject".

    The defaults are reasoned, not measured.  ``max_px`` = 0.5: the LK tracker
    stops when an iteration moves a point by less than ``track_precision`` =
    0.01 px, so a point at rest comes back within a few hundredths of a pixel
    of where it was; half a pixel is 50 termination steps above that floor and
    still below the one pixel at which the image itself resolves motion.
    ``min_tracks`` = 20: the default grid (4 x 5 cells, at least 3 features
    each) keeps 60 features or more, and 20 is one per cell -- below that the
    median stands on a few cells and one moving object can own it.  No
    reference counterpart."""
    max_px: float = 0.5
    quantile: float = 0.5
    min_tracks: int = 20
    mode: str = "veto"
    unknown: str = "imu"

    def __post_init__(self):
        if not float(self.max_px) >= 0.0:
            raise ValueError("VisionCue.max_px = %r must be >= 0" % (self.max_px,))
        if not 0.0 <= float(self.quantile) <= 1.0:
            raise ValueError("VisionCue.quantile = %r outside [0, 1]" % (self.quantile,))
        if int(self.min_tracks) < 1:
            raise ValueError("VisionCue.min_tracks = %r must be >= 1" % (self.min_tracks,))
        if self.mode not in _CUE_MODES:
            raise ValueError("VisionCue.mode = %r, expected one of %r" % (self.mode, _CUE_MODES))
        if self.unknown not in _CUE_UNKNOWNS:
            raise ValueError("VisionCue.unknown = %r, expected one of %r" % (self.unknown, _CUE_UNKNOWNS))

    def params(self):
        """The C-ABI's msckf_zupt_cue_t."""
        from ._lib import MsckfZuptCueT
        return MsckfZuptCueT(float(self.max_px), int(self.min_tracks), _CUE_MODES.index(self.mode),
                             _CUE_UNKNOWNS.index(self.unknown))


@dataclass
class ZuptConfig:
    """Parameters of the zero-velocity update (include/msckf_zupt.h): the noise
    variances of the three row groups, the gate on gamma (``chi2``; None: the
    reference's table at the kept rows' count, ``chi2_threshold(m)``), the gate
    on the speed and the groups kept.  ``vision`` (None or a ``VisionCue``):
    the front-end's track motion takes part in the decision
    (include/msckf_standstill.h).  No reference counterpart."""
    vel_noise: float = 1e-4
    gyro_noise: float = 4e-6
    acc_noise: float = 4e-4
    chi2: "float | None" = None
    max_speed: float = 0.1
    rows: tuple = ("vel", "gyro", "acc")
    vision: "VisionCue | None" = None

    def __post_init__(self):
        if self.vision is not None and not isinstance(self.vision, VisionCue):
            raise TypeError("ZuptConfig.vision must be a VisionCue or None, not %r" % (self.vision,))

    def mask(self) -> int:
        rows = (self.rows,) if isinstance(self.rows, str) else tuple(self.rows)
        m = 0
        for r in rows:
            if r not in _ZUPT_ROWS:
                raise ValueError("unknown ZUPT row group %r (one of %s)" % (r, ", ".join(_ZUPT_ROWS)))
            m |= _ZUPT_ROWS[r]
        if m == 0:
            raise ValueError("ZuptConfig.rows names no row group")
        return m

    def n_rows(self) -> int:
        return 3 * bin(self.mask()).count("1")

    def gate(self) -> float:
        return chi2_threshold(self.n_rows()) if self.chi2 is None else float(self.chi2)

    def params(self):
        """The C-ABI's msckf_zupt_params_t."""
        from ._lib import MsckfZuptParamsT
        return MsckfZuptParamsT(float(self.vel_noise), float(self.gyro_noise), float(self.acc_noise), self.gate(),
                                float(self.max_speed), self.mask())


AID_GROUPS = ("position", "velocity", "body_velocity", "direction")   # rows 3 g + axis (include/msckf_aid.h)
AID_TIME_TOL = 1e-9   # a delayed fix stamped this close to a clone's time is taken at the clone (lambda = 0)


def _orthonormal(R, what):
    R = np.asarray(R, float)
    if R.shape != (3, 3) or not (np.abs(R @ R.T - np.eye(3)).max() <= 1e-6):
        raise ValueError("%s must be a 3 x 3 orthonormal matrix (to 1e-6)" % what)
    return R


@dataclass
class AidingFix:
    """One aiding message: any of an antenna position and an IMU velocity (both
    in the external frame of ``AidingConfig.world_from_ext``), a velocity in the
    odometer frame and the reference direction as seen in the IMU frame, taken
    at ``timestamp``.  ``*_var``: the variance, a scalar or one per axis;
    ``*_axes``: which axes are used (a barometer is ``position`` with
    ``position_axes=(0, 0, 1)``).  ``received`` (optional) is the time the
    message reached the host: no frame before it sees the fix, so a replay can
    hand late messages over up front (``AidingConfig.delayed``)."""
    timestamp: float
    position: "np.ndarray | None" = None
    velocity: "np.ndarray | None" = None
    body_velocity: "np.ndarray | None" = None
    direction: "np.ndarray | None" = None
    position_var: "float | tuple" = 4e-4
    velocity_var: "float | tuple" = 4e-4
    body_velocity_var: "float | tuple" = 4e-4
    direction_var: "float | tuple" = 1e-4
    position_axes: tuple = (1, 1, 1)
    velocity_axes: tuple = (1, 1, 1)
    body_velocity_axes: tuple = (1, 1, 1)
    direction_axes: tuple = (1, 1, 1)
    received: "float | None" = None


@dataclass
class AidingConfig:
    """Parameters of the aiding fixes (include/msckf_aid.h): the antenna's lever
    arm in the IMU frame, the rotation IMU -> odometer frame, the reference
    direction in the filter's world frame, the gate on gamma (``chi2``; None: the
    upper 0.95 quantile ``CHI2_95`` at the kept rows' count, a float: that value
    for every count), the largest age at which a fix is still used, and
    ``world_from_ext`` = (R, t): external positions become R x + t and external
    velocities R v in the filter's world frame (gravity-aligned, origin and yaw
    set at initialisation).  No reference counterpart."""
    lever: tuple = (0.0, 0.0, 0.0)
    R_body: "np.ndarray" = field(default_factory=lambda: np.eye(3))
    dir_w: tuple = (1.0, 0.0, 0.0)
    chi2: "float | None" = None
    max_age: float = 0.05
    world_from_ext: tuple = field(default_factory=lambda: (np.eye(3), np.zeros(3)))
    # include/msckf_aid_delayed.h: a fix older than max_age is applied at its own timestamp, on the window's clones
    delayed: bool = False
    max_delay: float = 1.0    # the largest age of a delayed fix
    max_gap: float = 0.15     # the largest time between the two clones a delayed fix is interpolated between

    def gates(self):
        """The gate by the number of kept rows, 1..12."""
        return tuple(CHI2_95) if self.chi2 is None else (float(self.chi2),) * 12

    def check(self):
        if np.asarray(self.lever, float).shape != (3,) or not np.isfinite(np.asarray(self.lever, float)).all():
            raise ValueError("AidingConfig.lever must be three finite numbers")
        _orthonormal(self.R_body, "AidingConfig.R_body")
        d = np.asarray(self.dir_w, float)
        if d.shape != (3,) or not (abs(np.linalg.norm(d) - 1.0) <= 1e-6):
            raise ValueError("AidingConfig.dir_w must be a unit vector (to 1e-6)")
        if not (self.max_age >= 0.0):
            raise ValueError("AidingConfig.max_age = %r must be >= 0" % (self.max_age,))
        if not (self.max_delay >= 0.0) or not (self.max_gap > 0.0):
            raise ValueError("AidingConfig.max_delay = %r must be >= 0 and max_gap = %r > 0"
                             % (self.max_delay, self.max_gap))
        if np.isnan(self.gates()).any():
            raise ValueError("AidingConfig.chi2 is NaN")
        R, t = self.world_from_ext
        _orthonormal(R, "AidingConfig.world_from_ext's rotation")
        if np.asarray(t, float).shape != (3,):
            raise ValueError("AidingConfig.world_from_ext's translation must be three numbers")

    def params(self):
        """The C-ABI's msckf_aid_params_t."""
        from ._lib import MsckfAidParamsT
        self.check()
        p = MsckfAidParamsT()
        p.lever[:] = [float(x) for x in self.lever]
        p.R_body[:] = [float(x) for x in np.asarray(self.R_body, float).ravel()]
        p.dir_w[:] = [float(x) for x in self.dir_w]
        p.chi2[:] = self.gates()
        return p

    def rows_of(self, fix):
        """(z (12), var (12), mask) of an ``AidingFix`` in the filter's world
        frame; the entries of rows the fix does not carry are 0 / 1."""
        R, t = np.asarray(self.world_from_ext[0], float), np.asarray(self.world_from_ext[1], float)
        z, var, mask = np.zeros(12), np.ones(12), 0
        for g, name in enumerate(AID_GROUPS):
            val = getattr(fix, name)
            if val is None:
                continue
            val = np.asarray(val, float).reshape(3)
            if name == "position":
                val = R @ val + t
            elif name == "velocity":
                val = R @ val
            axes = tuple(getattr(fix, name + "_axes"))
            if len(axes) != 3:
                raise ValueError("AidingFix.%s_axes must have three entries" % name)
            z[3 * g:3 * g + 3] = val
            var[3 * g:3 * g + 3] = np.broadcast_to(np.asarray(getattr(fix, name + "_var"), float), (3,))
            for ax in range(3):
                if axes[ax]:
                    mask |= 1 << (3 * g + ax)
        return z, var, mask

    def merge(self, fixes, t_frame):
        """The fixes with t_frame - max_age <= timestamp <= t_frame merged into
        one measurement, each group from the newest fix that carries it:
        (z (12), var (12), dt, mask), or None if there is none.  dt is the age
        of the fix that gave the position rows (the only rows that use it), or
        of the newest fix without them."""
        z, var, mask, dt = np.zeros(12), np.ones(12), 0, None
        for fix in sorted((f for f in fixes if t_frame - self.max_age <= f.timestamp <= t_frame),
                          key=lambda f: -f.timestamp):
            zf, vf, mf = self.rows_of(fix)
            if dt is None and mf:
                dt = t_frame - fix.timestamp
            for g in range(4):
                grp = 7 << (3 * g)
                if (mf & grp) and not (mask & grp):
                    z[3 * g:3 * g + 3], var[3 * g:3 * g + 3] = zf[3 * g:3 * g + 3], vf[3 * g:3 * g + 3]
                    mask |= mf & grp
                    if g == 0:
                        dt = t_frame - fix.timestamp
        return (z, var, float(dt), mask) if mask else None

    def route(self, timestamp, mask, t_frame, cam_times):
        """Where a buffered fix (its timestamp <= t_frame and its 12-bit mask)
        goes at the frame t_frame, ``cam_times`` being the live clones' times,
        oldest first: ("current",) -- into ``merge``; ("delayed", slot, lambda,
        rows, dropped) -- include/msckf_aid_delayed.h's update on the clones
        ``slot`` and ``slot + 1`` with the 6-bit mask ``rows``, ``dropped`` the
        VEL / BVEL bits it cannot use; ("wait",) -- stale but newer than the
        newest clone, the next frame brackets it; ("drop", reason)."""
        age = t_frame - timestamp
        if age <= self.max_age:
            return ("current",)
        if not self.delayed:
            return ("drop", "stale")
        rows = (mask & 0x007) | (((mask >> 9) & 0x7) << 3)
        if not rows:
            return ("drop", "no delayed rows")
        if age > self.max_delay:
            return ("drop", "older than max_delay")
        if not len(cam_times) or timestamp < cam_times[0] - AID_TIME_TOL:
            return ("drop", "older than the window")
        if timestamp > cam_times[-1] + AID_TIME_TOL:
            return ("wait",)
        for s, ts in enumerate(cam_times):
            if abs(timestamp - ts) <= AID_TIME_TOL:
                return ("delayed", s, 0.0, rows, mask & 0x1f8)
        s = max(k for k, ts in enumerate(cam_times) if ts < timestamp)
        gap = cam_times[s + 1] - cam_times[s]
        if gap > self.max_gap + AID_TIME_TOL:
            return ("drop", "clones too far apart")
        return ("delayed", s, float((timestamp - cam_times[s]) / gap), rows, mask & 0x1f8)


ANCHOR_MAX = 64   # MSCKF_ANCHOR_MAX: anchors per filter and call (include/msckf_anchor.h)


@dataclass
class AnchorFix:
    """One anchor message: K points with known positions ``p`` (K, 3) in the
    external frame of ``AnchorConfig.world_from_ext``, their stereo observations
    ``z`` (K, 4) = (u0, v0, u1, v1) in the feature message's normalised
    coordinates, taken at ``timestamp``, and the positions' covariance ``cov``:
    a scalar variance, (K,) variances or (K, 3, 3)."""
    timestamp: float
    p: "np.ndarray"
    z: "np.ndarray"
    cov: "float | np.ndarray" = 1e-4

    def arrays(self):
        """(p (K, 3), z (K, 4), cov (K, 3, 3)), shapes checked."""
        p = np.asarray(self.p, float).reshape(-1, 3)
        z = np.asarray(self.z, float).reshape(-1, 4)
        K = len(p)
        if len(z) != K:
            raise ValueError("AnchorFix: %d points but %d observations" % (K, len(z)))
        c = np.asarray(self.cov, float)
        if c.ndim == 0:
            cov = np.broadcast_to(float(c) * np.eye(3), (K, 3, 3))
        elif c.shape == (K,):
            cov = c[:, None, None] * np.eye(3)
        elif c.shape == (K, 3, 3):
            cov = c
        else:
            raise ValueError("AnchorFix.cov must be a scalar, (K,) or (K, 3, 3), not %r" % (c.shape,))
        return p, z, cov


@dataclass
class AnchorConfig:
    """Parameters of the anchor fixes (include/msckf_anchor.h): the variance of a
    normalised coordinate (``obs_var``; None: the filter's
    ``observation_noise``), the per-anchor gate on gamma (``chi2``; None: the
    upper 0.95 quantile at four rows, ``CHI2_95[3]``), the least depth in both
    cameras, the least number of used anchors for an update, how far a message's
    timestamp may lie from its frame's, and ``world_from_ext`` = (R, t):
    external points become R x + t and their covariances R S R^T in the filter's
    world frame.  No reference counterpart."""
    obs_var: "float | None" = None
    chi2: "float | None" = None
    min_depth: float = 0.1
    min_anchors: int = 1
    time_tol: float = 1e-6
    world_from_ext: tuple = field(default_factory=lambda: (np.eye(3), np.zeros(3)))

    def gate(self):
        return CHI2_95[3] if self.chi2 is None else float(self.chi2)

    def check(self):
        if self.obs_var is not None and not (self.obs_var > 0.0 and np.isfinite(self.obs_var)):
            raise ValueError("AnchorConfig.obs_var = %r must be > 0" % (self.obs_var,))
        if np.isnan(self.gate()):
            raise ValueError("AnchorConfig.chi2 is NaN")
        if not (self.min_depth > 0.0 and np.isfinite(self.min_depth)):
            raise ValueError("AnchorConfig.min_depth = %r must be > 0" % (self.min_depth,))
        if int(self.min_anchors) != self.min_anchors or self.min_anchors < 1:
            raise ValueError("AnchorConfig.min_anchors = %r must be an integer >= 1" % (self.min_anchors,))
        if not (self.time_tol >= 0.0):
            raise ValueError("AnchorConfig.time_tol = %r must be >= 0" % (self.time_tol,))
        R, t = self.world_from_ext
        _orthonormal(R, "AnchorConfig.world_from_ext's rotation")
        if np.asarray(t, float).shape != (3,) or not np.isfinite(np.asarray(t, float)).all():
            raise ValueError("AnchorConfig.world_from_ext's translation must be three finite numbers")

    def params(self, observation_noise=None):
        """The C-ABI's msckf_anchor_params_t; ``observation_noise`` stands in for
        an ``obs_var`` of None."""
        from ._lib import MsckfAnchorParamsT
        self.check()
        var = self.obs_var if self.obs_var is not None else observation_noise
        if var is None:
            raise ValueError("AnchorConfig.obs_var is None and no observation_noise was given")
        return MsckfAnchorParamsT(float(var), self.gate(), float(self.min_depth), int(self.min_anchors))

    def in_world(self, fix):
        """(p (K, 3), cov (K, 3, 3), z (K, 4)) of an ``AnchorFix`` in the filter's
        world frame."""
        R, t = np.asarray(self.world_from_ext[0], float), np.asarray(self.world_from_ext[1], float)
        p, z, cov = fix.arrays()
        return p @ R.T + t, R @ cov @ R.T, z


@dataclass
class FilterConfig:
    """Filter fields of the reference ConfigEuRoC (config.py:17-124)."""
    optimization: OptimizationConfig = field(default_factory=OptimizationConfig)
    gravity: np.ndarray = field(default_factory=lambda: np.array([0.0, 0.0, -9.81]))
    max_cam_state_size: int = 20
    position_std_threshold: float = 8.0
    gyro_noise: float = 0.005 ** 2
    acc_noise: float = 0.05 ** 2
    gyro_bias_noise: float = 0.001 ** 2
    acc_bias_noise: float = 0.01 ** 2
    observation_noise: float = 0.035 ** 2
    velocity: np.ndarray = field(default_factory=lambda: np.zeros(3))
    velocity_cov: float = 0.25
    gyro_bias_cov: float = 0.01
    acc_bias_cov: float = 0.01
    extrinsic_rotation_cov: float = 3.0462e-4
    extrinsic_translation_cov: float = 2.5e-5
    T_imu_cam0: np.ndarray = field(default_factory=_default_T_imu_cam0)
    T_cn_cnm1: np.ndarray = field(default_factory=_default_T_cn_cnm1)
    T_imu_body: np.ndarray = field(default_factory=lambda: np.eye(4))

    @classmethod
    def from_reference(cls, ref_cfg) -> "FilterConfig":
        """Build from a reference-style config object (the attribute names the
        reference uses, config.py:9-124), so a caller holding a ConfigEuRoC
        can pass it straight through."""
        g = lambda n: getattr(ref_cfg, "_vio_%s__" % n)
        oc = g("optimization_config")
        go = lambda n: getattr(oc, "_vio_%s__" % n)
        return cls(
            optimization=OptimizationConfig(
                go("translation_threshold"), go("huber_epsilon"),
                go("estimation_precision"), go("initial_damping"),
                go("outer_loop_max_iteration"), go("inner_loop_max_iteration")),
            gravity=np.array(g("gravity"), float),
            max_cam_state_size=g("max_cam_state_size"),
            position_std_threshold=g("position_std_threshold"),
            gyro_noise=g("gyro_noise"), acc_noise=g("acc_noise"),
            gyro_bias_noise=g("gyro_bias_noise"), acc_bias_noise=g("acc_bias_noise"),
            observation_noise=g("observation_noise"),
            velocity=np.array(g("velocity"), float),
            velocity_cov=g("velocity_cov"), gyro_bias_cov=g("gyro_bias_cov"),
            acc_bias_cov=g("acc_bias_cov"),
            extrinsic_rotation_cov=g("extrinsic_rotation_cov"),
            extrinsic_translation_cov=g("extrinsic_translation_cov"),
            T_imu_cam0=np.array(g("T_imu_cam0"), float),
            T_cn_cnm1=np.array(g("T_cn_cnm1"), float),
            T_imu_body=np.array(g("T_imu_body"), float))
