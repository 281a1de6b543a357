"""Where the engine's switches live, CPU only: the engine-only ones are EngineConfig fields read by
from_env, the process-wide GEMM ones are globals of models/gemm_dispatch.py alone (a patch on a
stale copy in the engine module would silently test the default path), the engine module reads no
environment variable, and models/host_inputs.py imports without the engine or the ops."""
import subprocess
import sys
from dataclasses import fields

import pytest

from textsummarization_on_flink_amd.models.engine_config import EngineConfig

PKG = "textsummarization_on_flink_amd"
# (variable, field, value at "0", value at "1", value when unset): as the expressions these replace
# -- ``get(VAR, "1") != "0"`` for the five on by default, ``get(VAR, "0") == "1"`` for the two off
NEW_VARS = [("TSAMD_VOCAB_PAD", "vocab_pad", False, True, True),
            ("TSAMD_CTX_NATIVE", "ctx_native", False, True, True),
            ("TSAMD_DE_BF16", "de_bf16", False, True, True),
            ("TSAMD_DX_MERGE", "dx_merge", False, True, True),
            ("TSAMD_LSTM_FX", "lstm_fx", False, True, True),
            ("TSAMD_VOCAB_DW_SIDE", "vocab_dw_side", False, True, False),
            ("TSAMD_BLT_VOCAB_DW", "blt_vocab_dw", False, True, False)]


@pytest.mark.parametrize("var,field,at0,at1,unset", NEW_VARS)
def test_from_env_reads_the_engine_only_switches(var, field, at0, at1, unset):
    assert getattr(EngineConfig.from_env({var: "0"}), field) is at0
    assert getattr(EngineConfig.from_env({var: "1"}), field) is at1
    assert getattr(EngineConfig.from_env({}), field) is unset
    # any other value: still on for the five on by default, still off for the two that need "1"
    assert getattr(EngineConfig.from_env({var: "2"}), field) is unset
    assert getattr(EngineConfig.from_env({var: ""}), field) is unset


def test_from_env_defaults_are_the_dataclass_defaults():
    assert EngineConfig.from_env({}) == EngineConfig()
    assert EngineConfig().vocab_dw_split_min == 1e12
    assert EngineConfig.from_env({}, vocab_dw_split_min=0).vocab_dw_split_min == 0


def test_as_dict_lists_every_field():
    d = EngineConfig().as_dict()
    assert list(d) == [f.name for f in fields(EngineConfig)]
    assert {f for _, f, *_ in NEW_VARS} | {"vocab_dw_split_min"} <= set(d)


def test_host_inputs_imports_without_the_engine():
    code = (f"import sys, {PKG}.models.host_inputs\n"
            f"bad = [m for m in ('{PKG}.models.pointer_generator', '{PKG}.ops', '{PKG}.parallel.rccl_env')"
            " if m in sys.modules]\n"
            "assert not bad, bad\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_engine_module_reads_no_environment():
    from textsummarization_on_flink_amd.models import pointer_generator
    with open(pointer_generator.__file__) as f:
        src = f.read()
    assert "os.environ" not in src and "getenv" not in src


@pytest.mark.parametrize("name", ["GEMM_BT", "WGRAD_TT", "WGRAD_TT_MIN", "VOCAB_PAD", "CTX_NATIVE", "DE_BF16",
                                  "DX_MERGE", "LSTM_FX", "VOCAB_DW_SIDE", "VOCAB_DW_SPLIT_MIN", "BLT_WGRAD",
                                  "BLT_VDW"])
def test_engine_module_keeps_no_stale_switch(name):
    from textsummarization_on_flink_amd.models import gemm_dispatch, pointer_generator
    assert not hasattr(pointer_generator, name)
    # what bench.py reads there is the dispatch module's own object
    assert pointer_generator.BLT is gemm_dispatch.BLT
    assert pointer_generator.gemm_bt_stats is gemm_dispatch.gemm_bt_stats
