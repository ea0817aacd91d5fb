"""The engine's modules by role: spec and step_math import without torch or the ops front end, engine re-exports every name it had
when it was one file, and each module imports on its own (no cycles)."""
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "musicstyletransfer_amd"
MODULES = ("spec", "step_math", "params", "layer_block", "iw", "engine")

# what `engine` exposed as one file -> the module each name lives in now
HOMES = {
    "spec": ("VAEConfig", "positional_table", "logical_param_shapes", "xavier_init"),
    "params": ("ParamStore", "Dense", "Norm", "LayerParams"),
    "layer_block": ("Rows", "ALL_ROWS", "position0_rows", "Dropout", "NO_DROPOUT", "_Layer", "row_block_fwd", "_lead_mask", "no_partials",
                    "ffn_bwd_parts", "ffn_bwd_kw", "row_block_bwd", "layer_wgrads", "row_tail_selfcheck"),
    "step_math": ("roll_scores", "latent_scores", "iw_scores", "check_iw", "check_schedule", "check_clip", "check_input_dropout",
                  "check_ema", "clip_scale", "ema_decay_at", "ema_update", "schedule_values"),
    "engine": ("Forms", "StepPlan"),
    "iw": ("IWBound",),
    "ops": ("roundup",),
    "_lib": ("CE_MAX_WORKGROUPS", "ROLL_SLOTS"),
}


def _child(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_host_formulas_import_without_torch_or_ops():
    r = _child(f"import sys\n"
               f"from {PKG} import spec, step_math\n"
               f"assert 'torch' not in sys.modules, 'torch was imported'\n"
               f"assert '{PKG}.ops' not in sys.modules, 'ops was imported'\n"
               f"assert step_math.schedule_values(1, kl_warmup_steps=4) == (0.25, 1.0), step_math.schedule_values(1, kl_warmup_steps=4)\n")
    assert r.returncode == 0, r.stderr


def test_engine_reexports_every_name_it_had():
    engine = importlib.import_module(f"{PKG}.engine")
    assert engine.o is importlib.import_module(f"{PKG}.ops")
    for home, names in HOMES.items():
        mod = importlib.import_module(f"{PKG}.{home}")
        for name in names:
            assert hasattr(engine, name), f"engine.{name} is gone"
            assert getattr(engine, name) is getattr(mod, name), f"engine.{name} is not {home}.{name}"


def test_each_module_imports_on_its_own():
    """a fresh interpreter per module (started together: most of a child's time is importing torch)"""
    children = {m: subprocess.Popen([sys.executable, "-c", f"import importlib\nimportlib.import_module('{PKG}.{m}')\n"], cwd=ROOT,
                                    stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for m in MODULES}
    failed = {}
    for m, p in children.items():
        _, err = p.communicate(timeout=120)
        if p.returncode != 0:
            failed[m] = err
    assert not failed, "\n".join(f"{m}:\n{err}" for m, err in failed.items())
