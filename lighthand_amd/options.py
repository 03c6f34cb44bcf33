"""The plan-level switches (LH_* environment variables) as one value: ``PlanOptions``.

Every switch that decides WHICH launches a plan contains is a field of ``PlanOptions`` below; the field's declaration is the one
table of its environment name, its default (the value of an unset variable) and how the string is parsed.  ``Plan`` resolves the options
once (``PlanOptions.from_env()`` unless it is handed a set) and reads ``self.opt`` from there on; ``HipModule.plan``, ``TrainStep`` and
``InferStep`` pass an explicit set through (``options=`` / ``plan_options=``), and a variant is ``opt.replace(autotune=False)``.
The environment variables remain the outer interface of tests, tools and users.

NOT plan options -- process-level names, read where they are used, once per process or into class- / module-level state:
  LH_LIB_PATH          _lib.py: another build of the kernel library (kernel experiments).
  LH_TUNE_CACHE        tuner.py: the file measured choices persist in (0 / off / none: no persistence).
  LH_TUNE_DB           tuner.py: 0 ignores the shipped database, a path names another one.
  LH_TUNE_TIMES        tuner.py: a file that takes every timed candidate as a line (tools/ensemble_tune.py).
  XDG_CACHE_HOME       tuner.py: where the default tuning cache lives.
  LH_DIST_BACKEND      parallel.py: the torch.distributed backend (default nccl on a HIP device, else gloo).
  RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT    parallel.py, tools/train.py: the torchrun rendezvous.
and the switches the C library reads with getenv() itself:
  LH_POOL_STRIP        pool.hip: rows per strip of the BatchNorm + ReLU + max-pool forward (0: the window-per-thread kernel).
  LH_POOL_BLOCK        pool.hip: 0 runs the gated max-pool backward on the pixel-per-thread kernel.
  LH_BN_EXP            bn_common.h: bit flags of the cache-policy / traversal experiments of the streaming BatchNorm passes.
  LH_FOLD_IN_APPLY     fuse_bwd_plan.h: set (to anything), the backward apply pass no longer folds the partial sums itself.
  LH_DENSE_TILES       igemm_plan.hip: 0 withdraws the dense tile configurations from the candidates.
  LH_PW_OCC            igemm_pw_kernel.h: cap on the pointwise kernel's workgroups per compute unit (default 4).
  LH_WGRAD_TABLE_XCD   wgrad_table.hip: 0 orders a table's work items longest first without dealing them over the XCDs.
"""
import dataclasses
import os
from dataclasses import dataclass


def _on(v):
    """on/off: off only when the value is the string "0"."""
    return v != "0"


def _int_tuple(v):
    return tuple(int(t) for t in v.split(",")) if v else None


def _l2_touch(v):
    return {"0": 0, "2": 2}.get(v, 1)


def _sw(env, default, parse=_on):
    return dataclasses.field(default=default, metadata={"env": env, "parse": parse})


@dataclass(frozen=True)
class PlanOptions:
    # ---- the autotuner (tuner.py)
    autotune: bool = _sw("LH_AUTOTUNE", True)                         # off: the library's static defaults, nothing is measured
    tune_cold: bool = _sw("LH_TUNE_COLD", True)                       # off: time launches back to back (_tune, _tune_wgrad)
    tune_iters: int = _sw("LH_TUNE_ITERS", 4, lambda v: max(1, int(v)))    # timed launches per candidate (tools/make_tune_db.sh: 20)
    tune_log: bool = _sw("LH_TUNE_LOG", False, bool)                  # a line per timed candidate
    wgrad_table_log: bool = _sw("LH_WGRAD_TABLE_LOG", False, bool)    # ... of the table launches
    # ---- merged launches of HRNet's branches, the weight-gradient schedule
    batch: bool = _sw("LH_BATCH", True)                               # off: stream lanes instead of batch groups
    wgrad_batch: bool = _sw("LH_WGRAD_BATCH", True)
    wgrad_table: bool = _sw("LH_WGRAD_TABLE", True)                   # off: one launch (+ fold) per layer
    wgrad_table_big: bool = _sw("LH_WGRAD_TABLE_BIG", True)           # the 256 x 256 tile class
    wgrad_table_stragglers: bool = _sw("LH_WGRAD_TABLE_STRAGGLERS", True)    # a layer alone in its class joins the nearest table
    wgrad_table_force: tuple = _sw("LH_WGRAD_TABLE_FORCE", None, _int_tuple)  # "bo,bi,kps,depth,target" for every table
    wgrad_table_tune_min: int = _sw("LH_WGRAD_TABLE_TUNE_MIN", 20000, int)    # tables with less work are not measured
    wgrad_group: int = _sw("LH_WGRAD_GROUP", None, int)               # layers per deferred group; None: Plan's rule, 0: in place
    wgrad_lanes: int = _sw("LH_WGRAD_LANES", None, int)               # weight-gradient streams; None: Plan's rule
    # ---- the BatchNorm-backward gate (lh_igemm_gated), caps in MiB
    bn_gate: bool = _sw("LH_BN_GATE", True)
    bn_gate_pw: bool = _sw("LH_BN_GATE_PW", True)                     # the pointwise kernel's epilogue takes the gate too
    bn_gate_tail: bool = _sw("LH_BN_GATE_TAIL", True)                 # residual tails (sign from the stored mask bits)
    bn_gate_tail2: bool = _sw("LH_BN_GATE_TAIL2", True)               # ... tails with a projection shortcut (two BatchNorm terms)
    bn_gate_branches: bool = _sw("LH_BN_GATE_BRANCHES", True)         # ... in networks with parallel branches, outside the branch regions
    bn_gate_max_mb: float = _sw("LH_BN_GATE_MAX_MB", 9.0, float)
    bn_gate_pw_max_mb: float = _sw("LH_BN_GATE_PW_MAX_MB", 1024.0, float)
    bn_gate_tail_max_mb: float = _sw("LH_BN_GATE_TAIL_MAX_MB", 1024.0, float)
    bn_gate_tiled_tail_max_mb: float = _sw("LH_BN_GATE_TILED_TAIL_MAX_MB", 1024.0, float)
    # ---- single rewrites of the launch lists
    late_pack: bool = _sw("LH_LATE_PACK", True)                       # second weight-pack launch under the middle of the forward pass
    tail_spread: bool = _sw("LH_TAIL_SPREAD", True)                   # the last deferred group over all weight-gradient streams
    stem_direct: bool = _sw("LH_STEM_DIRECT", True)                   # the training stem on lh_stem_conv
    bn_pool: bool = _sw("LH_BN_POOL", True)                           # BatchNorm + ReLU inside the max-pool forward
    pool_gate: bool = _sw("LH_POOL_GATE", True)                       # the gate in the max-pool backward
    fuse_bottleneck: bool = _sw("LH_FUSE_BOTTLENECK", True)           # stage-1 bottlenecks of inference plans as one launch
    l2_touch: int = _sw("LH_L2_TOUCH", 1, _l2_touch)                  # 0 off, 1 on, 2 the persistent kernels' panels too
    l2_touch_max_mb: float = _sw("LH_L2_TOUCH_MAX_MB", 3.0, float)

    @classmethod
    def from_env(cls, environ=os.environ):
        """The options a mapping of environment variables asks for (nothing but `environ` is read)."""
        return cls(**{f.name: f.metadata["parse"](environ[f.metadata["env"]]) for f in dataclasses.fields(cls) if f.metadata["env"] in environ})

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)
