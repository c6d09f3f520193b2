"""Host: `Switches.from_env` -- the one place the decoder's and the Q-Formers' A/B switches are read from the environment."""
import dataclasses
import pathlib
import re

import pytest

from unirec_amd.switches import Switches, switches

ON_UNLESS_0 = {"merge_proj": "UNIREC_MERGE_PROJ", "fuse_norm_lora": "UNIREC_FUSE_NORM_LORA", "fuse_qk_rope": "UNIREC_FUSE_QK_ROPE",
               "fuse_swiglu_gemm": "UNIREC_FUSE_SWIGLU_GEMM", "fuse_swiglu_lora": "UNIREC_FUSE_SWIGLU_LORA", "bits_t": "UNIREC_BITS_T",
               "bits_next": "UNIREC_BITS_NEXT", "pad_att": "UNIREC_PAD_ATT", "rope_k_fused": "UNIREC_ROPE_K_FUSED", "kv_colsum": "UNIREC_KV_COLSUM",
               "qf_wt": "UNIREC_QF_WT", "qf_dw_stream": "UNIREC_QF_DW_STREAM", "qf_dw_grouped": "UNIREC_QF_DW_GROUPED"}
OFF_UNLESS_1 = {"swiglu_fwd_fused": "UNIREC_SWIGLU_FWD_FUSED", "recompute_mlp": "UNIREC_RECOMPUTE_MLP", "bits_one_event": "UNIREC_BITS_ONE_EVENT"}
THREE_VALUED = {"rope_bwd_fused": "UNIREC_ROPE_BWD_FUSED"}
ALL = {**ON_UNLESS_0, **OFF_UNLESS_1, **THREE_VALUED}


def test_every_field_has_its_variable():
    assert Switches.variables() == ALL
    assert {f.name for f in dataclasses.fields(Switches)} == set(ALL)
    assert isinstance(switches, Switches)


def test_defaults_for_an_empty_mapping():
    s = Switches.from_env({})
    assert s == Switches()
    for field in ON_UNLESS_0:
        assert getattr(s, field) is True, field
    for field in OFF_UNLESS_1:
        assert getattr(s, field) is False, field
    assert s.rope_bwd_fused is None


@pytest.mark.parametrize("field", list(ALL))
def test_zero_and_one_of_each_variable(field):
    var = ALL[field]
    for value, want in (("0", False), ("1", True)):
        s = Switches.from_env({var: value})
        assert getattr(s, field) is want, (var, value)
        for other in ALL:          # ... and no other field moves
            if other != field:
                assert getattr(s, other) == getattr(Switches(), other), (var, value, other)


@pytest.mark.parametrize("field", list(ON_UNLESS_0) + list(OFF_UNLESS_1))
@pytest.mark.parametrize("value", ["", "2", "true", "off", " 0"])
def test_any_other_value_is_the_default(field, value):
    assert getattr(Switches.from_env({ALL[field]: value}), field) is getattr(Switches(), field)


@pytest.mark.parametrize("value,want", [("0", False), ("1", True), ("2", None), ("", None), ("true", None)])
def test_rope_bwd_fused_is_three_valued(value, want):
    assert Switches.from_env({"UNIREC_ROPE_BWD_FUSED": value}).rope_bwd_fused is want
    assert Switches.from_env({}).rope_bwd_fused is None


def test_from_env_reads_nothing_but_its_mapping(monkeypatch):
    monkeypatch.setenv("UNIREC_MERGE_PROJ", "0")
    assert Switches.from_env({}).merge_proj is True


def test_readme_table_names_the_same_variables():
    readme = (pathlib.Path(__file__).resolve().parent.parent / "README.md").read_text()
    section = readme.split("\n## Switches", 1)[1].split("\n## ", 1)[0]
    tables = [blk for blk in section.split("\n\n") if blk.startswith("| Variable |")]          # the table of the fields of `switches`
    assert len(tables) == 1
    table = tables[0]
    assert set(re.findall(r"UNIREC_[A-Z0-9_]+", table)) == set(ALL.values())


def test_the_decoder_and_the_qformers_do_not_read_the_environment():
    pkg = pathlib.Path(__file__).resolve().parent.parent / "unirec_amd"
    for name in ("qwen3.py", "qformer.py"):
        assert "os.environ" not in (pkg / name).read_text(), name
