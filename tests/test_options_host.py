"""lighthand_amd.options.PlanOptions: defaults, parse rules, hashing -- and that no other module of the package reads a plan-level
LH_* switch from the environment (CPU only)."""
import dataclasses
import pathlib
import re

import pytest

from lighthand_amd.options import PlanOptions

# the defaults of an empty environment, written out (NOT derived from the table under test)
DEFAULTS = dict(
    autotune=True, tune_cold=True, tune_iters=4, tune_log=False, wgrad_table_log=False,
    batch=True, wgrad_batch=True, wgrad_table=True, wgrad_table_big=True, wgrad_table_stragglers=True,
    wgrad_table_force=None, wgrad_table_tune_min=20000, wgrad_group=None, wgrad_lanes=None,
    bn_gate=True, bn_gate_pw=True, bn_gate_tail=True, bn_gate_tail2=True, bn_gate_branches=True,
    bn_gate_max_mb=9.0, bn_gate_pw_max_mb=1024.0, bn_gate_tail_max_mb=1024.0, bn_gate_tiled_tail_max_mb=1024.0,
    late_pack=True, tail_spread=True, stem_direct=True, bn_pool=True, pool_gate=True, fuse_bottleneck=True,
    l2_touch=1, l2_touch_max_mb=3.0)

ENV_NAMES = dict(
    autotune="LH_AUTOTUNE", tune_cold="LH_TUNE_COLD", tune_iters="LH_TUNE_ITERS", tune_log="LH_TUNE_LOG", wgrad_table_log="LH_WGRAD_TABLE_LOG",
    batch="LH_BATCH", wgrad_batch="LH_WGRAD_BATCH", wgrad_table="LH_WGRAD_TABLE", wgrad_table_big="LH_WGRAD_TABLE_BIG",
    wgrad_table_stragglers="LH_WGRAD_TABLE_STRAGGLERS", wgrad_table_force="LH_WGRAD_TABLE_FORCE", wgrad_table_tune_min="LH_WGRAD_TABLE_TUNE_MIN",
    wgrad_group="LH_WGRAD_GROUP", wgrad_lanes="LH_WGRAD_LANES",
    bn_gate="LH_BN_GATE", bn_gate_pw="LH_BN_GATE_PW", bn_gate_tail="LH_BN_GATE_TAIL", bn_gate_tail2="LH_BN_GATE_TAIL2",
    bn_gate_branches="LH_BN_GATE_BRANCHES", bn_gate_max_mb="LH_BN_GATE_MAX_MB", bn_gate_pw_max_mb="LH_BN_GATE_PW_MAX_MB",
    bn_gate_tail_max_mb="LH_BN_GATE_TAIL_MAX_MB", bn_gate_tiled_tail_max_mb="LH_BN_GATE_TILED_TAIL_MAX_MB",
    late_pack="LH_LATE_PACK", tail_spread="LH_TAIL_SPREAD", stem_direct="LH_STEM_DIRECT", bn_pool="LH_BN_POOL", pool_gate="LH_POOL_GATE",
    fuse_bottleneck="LH_FUSE_BOTTLENECK", l2_touch="LH_L2_TOUCH", l2_touch_max_mb="LH_L2_TOUCH_MAX_MB")

ON_OFF = [k for k, v in DEFAULTS.items() if v is True]
MIB = [k for k in DEFAULTS if k.endswith("_max_mb")]


def test_defaults_of_an_empty_environment():
    opt = PlanOptions.from_env({})
    assert {f.name for f in dataclasses.fields(opt)} == set(DEFAULTS)
    for name, want in DEFAULTS.items():
        got = getattr(opt, name)
        assert got == want and type(got) is type(want), (name, got, want)
    assert opt == PlanOptions()
    assert {f.name: f.metadata["env"] for f in dataclasses.fields(opt)} == ENV_NAMES


@pytest.mark.parametrize("field", ON_OFF)
def test_on_off_fields_are_off_only_for_the_string_zero(field):
    assert len(ON_OFF) == 18
    env = ENV_NAMES[field]
    assert getattr(PlanOptions.from_env({env: "0"}), field) is False
    for v in ("1", "2", "yes", "", "00", "off"):
        assert getattr(PlanOptions.from_env({env: v}), field) is True, (field, v)
    assert PlanOptions.from_env({env: "0"}) == PlanOptions().replace(**{field: False})     # and no other field moved


def test_parse_rules_of_the_other_fields():
    f = PlanOptions.from_env
    assert [f({"LH_L2_TOUCH": v}).l2_touch for v in ("0", "1", "2", "3", "yes")] == [0, 1, 2, 1, 1]
    assert [f({"LH_TUNE_ITERS": v}).tune_iters for v in ("0", "-3", "1", "20")] == [1, 1, 1, 20]
    assert f({"LH_WGRAD_GROUP": "0"}).wgrad_group == 0 and f({"LH_WGRAD_GROUP": "0"}).wgrad_group is not None
    assert f({"LH_WGRAD_GROUP": "24"}).wgrad_group == 24
    assert f({"LH_WGRAD_LANES": "3"}).wgrad_lanes == 3
    assert f({"LH_WGRAD_TABLE_FORCE": "128,128,64,2,4"}).wgrad_table_force == (128, 128, 64, 2, 4)
    assert f({"LH_WGRAD_TABLE_FORCE": ""}).wgrad_table_force is None
    assert f({"LH_WGRAD_TABLE_TUNE_MIN": "0"}).wgrad_table_tune_min == 0
    for name in MIB:
        assert getattr(f({ENV_NAMES[name]: "1.5"}), name) == 1.5
        assert getattr(f({ENV_NAMES[name]: "12"}), name) == 12.0
    assert len(MIB) == 5
    for name in ("tune_log", "wgrad_table_log"):                                  # set and non-empty
        assert getattr(f({ENV_NAMES[name]: "1"}), name) is True
        assert getattr(f({ENV_NAMES[name]: "0"}), name) is True
        assert getattr(f({ENV_NAMES[name]: ""}), name) is False
    with pytest.raises(ValueError):
        f({"LH_WGRAD_GROUP": "many"})


def test_from_env_reads_only_the_mapping_it_is_given(monkeypatch):
    for env in ENV_NAMES.values():
        monkeypatch.setenv(env, "0")
    assert PlanOptions.from_env({}) == PlanOptions()
    assert PlanOptions.from_env({"LH_BATCH": "0"}) == PlanOptions(batch=False)
    got = PlanOptions.from_env()                                                  # the default mapping is the process environment
    assert not got.autotune and not got.bn_gate and got.l2_touch == 0 and got.wgrad_group == 0 and got.tune_iters == 1
    monkeypatch.setenv("LH_AUTOTUNE", "1")                                        # ... as it is at the call, not at import
    assert PlanOptions.from_env().autotune


def test_options_are_hashable_values():
    a, b = PlanOptions.from_env({"LH_BN_GATE_MAX_MB": "4", "LH_WGRAD_TABLE_FORCE": "64,64,64,3,0"}), \
        PlanOptions.from_env({"LH_WGRAD_TABLE_FORCE": "64,64,64,3,0", "LH_BN_GATE_MAX_MB": "4.0"})
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    c = a.replace(autotune=False)
    assert c != a and len({a, c}) == 2
    diff = [f.name for f in dataclasses.fields(a) if getattr(a, f.name) != getattr(c, f.name)]
    assert diff == ["autotune"]
    assert a.autotune                                                             # replace() makes a variant, the original is frozen
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.autotune = False


# process-level names: read once per process, where they are used (options.py's docstring says what each is)
PROCESS_LEVEL = {"LH_LIB_PATH", "LH_TUNE_CACHE", "LH_TUNE_DB", "LH_TUNE_TIMES", "LH_DIST_BACKEND"}
# an ACCESS of the environment that names an LH_* variable: os.environ.get("LH_X" / os.environ["LH_X" / os.getenv("LH_X" /
# os.environ.pop / setdefault, and "LH_X" in os.environ -- a comment or docstring that merely mentions a switch does not match
ACCESS = re.compile(r"""(?:environ\s*(?:\.\s*\w+\s*\(|\[)|getenv\s*\()\s*f?["'](LH_[A-Z0-9_]*)|["'](LH_[A-Z0-9_]*)["']\s+(?:not\s+)?in\s+(?:os\s*\.\s*)?environ""")


def test_the_access_pattern_matches_what_it_should():
    hits = lambda s: [a or b for a, b in ACCESS.findall(s)]
    assert hits('x = os.environ.get("LH_BATCH", "1") != "0"') == ["LH_BATCH"]
    assert hits("os.environ['LH_AUTOTUNE'] = '0'") == ["LH_AUTOTUNE"]
    assert hits('os.getenv("LH_TUNE_LOG")') == ["LH_TUNE_LOG"]
    assert hits('os.environ.pop("LH_AUTOTUNE", None)') == ["LH_AUTOTUNE"]
    assert hits('if "LH_TUNE_CACHE" not in os.environ:') == ["LH_TUNE_CACHE"]
    assert hits('environ.setdefault( "LH_X", "1")') == ["LH_X"]
    assert hits("# LH_BATCH=0 keeps the lanes (os.environ is not read here)") == []
    assert hits('"""LH_TUNE_TIMES=<file>: every timed candidate"""') == []


def test_no_plan_level_switch_is_read_outside_options():
    root = pathlib.Path(__file__).resolve().parent.parent / "lighthand_amd"
    files = sorted(root.rglob("*.py"))
    assert len(files) > 10 and root / "engine.py" in files and root / "tools" / "train.py" in files
    found = {}
    for path in files:
        if path.name == "options.py" and path.parent == root:
            continue
        for a, b in ACCESS.findall(path.read_text()):
            found.setdefault(a or b, set()).add(str(path.relative_to(root)))
    stray = {k: sorted(v) for k, v in found.items() if k not in PROCESS_LEVEL}
    assert not stray, f"LH_* switches read from the environment outside options.py: {stray}"
    assert set(found) >= {"LH_LIB_PATH", "LH_TUNE_CACHE", "LH_TUNE_DB"}          # the scan does see the reads that remain
