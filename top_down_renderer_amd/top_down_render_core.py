"""TopDownRenderCore — the ROS-free part of the reference's orchestrator `TopDownRender`
(include/top_down_render/top_down_render.h:36-108, src/top_down_render.cpp) over the Python classes of this package: what
the node does with the hot-path classes once a cloud and a motion prior have arrived.  The C++ form of the same class is
include/top_down_render/top_down_render_core.h; both follow

    initialize      :81, 115-117   samplePtsPolar(100 x 25) / ParticleFilter / ScanRendererPolar
    takeStep        :505-560       render at current_range_scale_, updateFilter, publishPoseEst
    updateFilter    :413-425       propagate(trans, yaw), update(top_down, top_down_geo, res)
    publishPoseEst  :331-365       range-scale stepping (+0.05 / -0.02 inside [range_scale_min_, range_scale_max_]), the
                                   freezeScale trigger (cov(3,3) < 0.003 scale), the convergence gate

The node changes `res` on EVERY step, so a filter is scored with a different range scale scan after scan
(tests/test_takestep_loop.py).  The scan stays on the device between the renderer and the filter."""
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .particle_filter import KldParams, ParticleFilter, RecoveryParams, kld_params_c, recovery_params_c
from .scan_renderer import ScanRendererPolar


@dataclass
class CoreConfig:                       # the node's parameters that reach the step (src/top_down_render.cpp:45-53)
    particle_count: int = 20000         # :53
    range_scale_min: float = 0.5        # :45
    range_scale_max: float = 4.0        # :46
    target_uncertainty_m: float = 2.5   # top_down_render.h:80
    theta_bins: int = 100               # hard-coded 100 x 25 in the node (:115, 530, 534); parameters here
    range_bins: int = 25
    seed: int = 0                       # ParticleFilter's seed
    # the adaptive particle count (src/particle_filter.cpp:151-157): after the publishPoseEst of every gmm_every-th step
    # the mixture is refitted on the device and every update resamples to the count of :151-157.  0: never
    gmm_every: int = 0
    # KLD-sampling count (include/tdr.h, "KLD-sampling count"): after the publishPoseEst of every kld_every-th step the pose
    # bins of the particle set are counted on the device and the following updates resample to the count they ask for.
    # 0: never.  Together with gmm_every > 0 it is refused: two rules for one number
    kld_every: int = 0
    kld: KldParams = field(default_factory=KldParams)
    # recovery injection (include/tdr.h, "recovery injection"): after the publishPoseEst of every recovery_every-th step the
    # slow / fast averages take the update's mean raw weight and, when the fast one has dropped below the slow one, fresh
    # on-road particles replace that share of the slots (the step's estimate is the un-injected set's).  0: never
    recovery_every: int = 0
    recovery: RecoveryParams = field(default_factory=RecoveryParams)
    # sensor resetting (include/tdr.h, "sensor resetting"): above 1, a due recovery step gives every injected slot the
    # best-scoring of this many road candidates against the step's render at the step's res.  1: the plain injection
    recovery_candidates: int = 1

    def check(self):
        if self.recovery_every > 0:
            recovery_params_c(self.recovery)
            if not 1 <= int(self.recovery_candidates) <= 4096:
                raise ValueError("CoreConfig: recovery_candidates must lie in 1 .. 4096")
        if self.kld_every > 0 and self.gmm_every > 0:
            raise ValueError("CoreConfig: kld_every and gmm_every are two rules for one particle count; set one of them")
        if self.kld_every > 0:
            kld_params_c(self.kld)


@dataclass
class PoseEst:                          # what publishPoseEst computed this step
    cov: np.ndarray = field(default_factory=lambda: np.zeros((4, 4), np.float32))   # computeMeanCov (:333)
    ml_state: np.ndarray = None         # meanLikelihood (:354); None when the filter holds no particle (:347-350)
    scale: float = -1.0                 # filter_->scale() at :335
    range_scale: float = 0.0            # current_range_scale_ AFTER the step's adjustment: the next scan's res
    froze_scale: bool = False           # freezeScale() was called in this step (:356-359)
    converged: bool = False             # is_converged_ (:362-364; sticky)


class TopDownRenderCore:
    def __init__(self, cfg=None, kernels=None):
        self.cfg = cfg or CoreConfig()
        self.k = kernels
        self.current_range_scale_ = np.float32(self.cfg.range_scale_max)   # :47
        self.last_res_ = np.float32(0)
        self.is_converged_ = False                                         # top_down_render.h:83
        self.map_ = self.filter_ = self.renderer_ = None
        self.steps_ = 0                                                    # counted only with cfg.gmm_every / kld_every > 0
        self.kld_target_ = None                                            # the count the last kldCount asked for
        self.recovery_steps_ = 0                                           # counted only with cfg.recovery_every > 0
        self.recovery_state_ = _lib.RecoveryStateC(0.0, 0.0)
        self.last_recovery_ = (0.0, 0)                                     # (p, injected) of the last recovery step

    def initialize(self, map, filter_params, flatten_lut, **filter_kw):
        """:81, 115-117 with a TopDownMapPolar the host built."""
        c = self.cfg
        c.check()
        self.map_ = map
        self.steps_ = 0
        self.kld_target_ = None
        self.recovery_steps_ = 0
        self.recovery_state_ = _lib.RecoveryStateC(0.0, 0.0)
        self.ang_res = np.float32(2 * np.pi / c.theta_bins)
        map.samplePtsPolar((c.theta_bins, c.range_bins), self.ang_res)                                     # :115
        self.filter_ = ParticleFilter(c.particle_count, map, filter_params, seed=c.seed, kernels=self.k, **filter_kw)   # :116
        self.renderer_ = ScanRendererPolar(flatten_lut, kernels=self.k)                                    # :117
        self.renderer_.set_output_shape(map.numClasses(), c.theta_bins, c.range_bins)

    def takeStep(self, cloud, trans, yaw):
        """takeStep (:505-560).  trans / yaw: the motion prior's delta projected to the plane like updateFilter does
        (:418-420, projectPrior).  Returns the step's PoseEst, or None when the step was skipped (no map yet, :508-511)."""
        if self.map_ is None or not self.map_.haveMap():
            return None
        self.last_res_ = self.current_range_scale_
        self.renderer_.renderSemanticTopDown(cloud, float(self.current_range_scale_), self.ang_res)         # :539
        self.updateFilter(self.renderer_.last_scan(), None, float(self.current_range_scale_), trans, yaw)   # :559
        e = self.publishPoseEst()                                                                           # :560
        if self.countStepAndGmmDue():
            self.filter_.computeGMM(device=True)
        if self.countStepAndKldDue():
            self.kld_target_ = self.filter_.kldCount(self.cfg.kld)
        if self.countStepAndRecoveryDue():
            if self.cfg.recovery_candidates > 1:
                self.last_recovery_ = self.filter_.recoveryStepSensor(self.recovery_state_, self.cfg.recovery,
                                                                      self.cfg.recovery_candidates, self.renderer_.last_scan(),
                                                                      float(self.last_res_))
            else:
                self.last_recovery_ = self.filter_.recoveryStep(self.recovery_state_, self.cfg.recovery)
        return e

    def countStepAndGmmDue(self):
        """Counts the step AND says whether its mixture fit is due (cfg.gmm_every): exactly one call per step."""
        g = self.cfg.gmm_every
        if g <= 0:
            return False
        self.steps_ += 1
        return self.steps_ % g == 0

    def countStepAndKldDue(self):
        """The same for the KLD-sampling count (cfg.kld_every; never both, CoreConfig.check)."""
        g = self.cfg.kld_every
        if g <= 0:
            return False
        self.steps_ += 1
        return self.steps_ % g == 0

    def countStepAndRecoveryDue(self):
        """The same for the recovery injection (cfg.recovery_every), on a counter of its own."""
        g = self.cfg.recovery_every
        if g <= 0:
            return False
        self.recovery_steps_ += 1
        return self.recovery_steps_ % g == 0

    def updateFilter(self, top_down, top_down_geo, res, trans, yaw):
        self.filter_.propagate(trans, yaw)                                                                  # :423
        if self.cfg.gmm_every > 0:   # :151-157 from the clusters of the last fit
            self.filter_.update(top_down, top_down_geo, res, n_target=self.filter_.adaptiveCount())
        elif self.cfg.kld_every > 0 and self.kld_target_ is not None:   # the count the bins of the last kldCount asked for
            self.filter_.update(top_down, top_down_geo, res, n_target=self.kld_target_)
        else:
            self.filter_.update(top_down, top_down_geo, res)                                                # :425

    def publishPoseEst(self):
        """publishPoseEst (:331-365) without the publishing."""
        f, c = self.filter_, self.cfg
        e = PoseEst()
        e.cov = np.asarray(f.computeMeanCov(), np.float32)                                                  # :333
        scale = np.float32(f.scale())                                                                       # :335
        scale_2 = np.float32(scale * scale)
        e.scale = float(scale)
        spread = np.float32(max(e.cov[0, 0], e.cov[1, 1]) / scale_2)
        # (the node compares against std::pow(float, int), a double, and steps its float member by double constants)
        if float(spread) > float(np.float32(c.target_uncertainty_m)) ** 2 and self.current_range_scale_ < np.float32(c.range_scale_max):
            self.current_range_scale_ = np.float32(np.float64(self.current_range_scale_) + 0.05)             # :341 widen
        elif self.current_range_scale_ > np.float32(c.range_scale_min):
            self.current_range_scale_ = np.float32(np.float64(self.current_range_scale_) - 0.02)             # :344 shrink
        e.range_scale = float(self.current_range_scale_)
        e.converged = self.is_converged_
        if f.numParticles() < 1:                                                                            # :347-350
            return e
        e.ml_state = np.asarray(f.meanLikelihood(), np.float32)                                             # :354
        if float(e.cov[3, 3]) < 0.003 * float(e.ml_state[3]) and not f.isScaleFrozen():                      # :356
            f.freezeScale()                                                                                 # :359
            e.froze_scale = True
        if (np.float32(e.cov[0, 0] / scale_2) < 40 and np.float32(e.cov[1, 1] / scale_2) < 40 and e.cov[2, 2] < 0.5
                and f.scale() > 0):                                                                         # :363
            self.is_converged_ = True
        e.converged = self.is_converged_
        return e

    @staticmethod
    def projectPrior(R, t):
        """The plane projection of a 3-D motion prior (updateFilter, :418-420): R 3 x 3, t the translation."""
        R = np.asarray(R, np.float32).reshape(3, 3)
        return (float(t[0]), float(t[1])), float(np.arctan2(R[1, 0], R[0, 0]))

    def currentRangeScale(self):
        return float(self.current_range_scale_)

    def lastRes(self):
        return float(self.last_res_)

    def isConverged(self):
        return self.is_converged_
