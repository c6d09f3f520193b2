"""CPU: every entry point declared in include/unirec_hip.h or in one of the family headers include/unirec_*.h (include/unirec_fp8.h among them) is either listed in a COVERS table -- naming the primitive-level test(s)
that hold it against a reference -- or exempt below with a reason.  A new entry point without such a test fails here."""
import ast
import functools
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERS_MODULES = ("tests/test_gpu_primitives.py", "tests/test_gpu_head_primitives.py", "tests/test_gpu_attention_f64.py", "tests/test_gpu_norm_f64.py",
                  "tests/test_gpu_lora_f64.py", "tests/test_gpu_gemm_f64.py", "tests/test_gpu_elementwise_f64.py", "tests/test_gpu_dw_f64.py",
                  # the family headers: catalogue retrieval and losses, Matryoshka, pooling, LoRA merge
                  "tests/test_gpu_catalog_deep.py", "tests/test_gpu_catalog_coarse.py", "tests/test_gpu_catalog_coarse_deep.py",
                  "tests/test_gpu_catalog_funnel.py", "tests/test_gpu_catalog_softmax.py", "tests/test_gpu_catalog_mrl_softmax.py",
                  "tests/test_gpu_mrl_f64.py", "tests/test_gpu_pool_f64.py", "tests/test_gpu_lora_merge.py",
                  # where the catalogue calls read and write: the weakest alignments, guards, poisoned workspaces; rows past 4 GiB
                  "tests/test_gpu_catalog_memory.py", "tests/test_gpu_catalog_4gib.py",
                  # the FP8 catalogues of include/unirec_fp8.h
                  "tests/test_gpu_catalog_fp8.py", "tests/test_gpu_catalog_fp8_memory.py",
                  # where the training hot path reads and writes: GEMM, attention, LoRA under the same memory contract
                  "tests/test_gpu_gemm_memory.py", "tests/test_gpu_attention_memory.py", "tests/test_gpu_lora_memory.py")

EXEMPT = {
    "ur_version": "ABI handshake; asserted at every library load (unirec_amd/_lib.py) and in tests/test_cabi.py",
    "ur_last_error": "error text; read by every rejected call the GPU tests provoke",
    "ur_gemm_workspace_bytes": "workspace-size query; a short workspace is rejected by ur_gemm",
    "ur_gemm_grouped_workspace_bytes": "workspace-size query",
    "ur_lora_bits_ld": "layout query (bytes per row of a bit plane)",
    "ur_lora_bits_t_ld": "layout query (words per token group)",
    "ur_lora_reduce_workspace_bytes": "workspace-size query",
    "ur_lora_bgrad_workspace_bytes": "workspace-size query",
    "ur_layernorm_bwd_workspace_bytes": "workspace-size query",
    "ur_batch_reduce_workspace_bytes": "workspace-size query",
    "ur_attn_bwd_workspace_floats": "workspace-size query",
    "ur_attn_bwd_kv_colsum_floats": "workspace-size / capability query (tests/test_gpu_r5_parity.py exercises both answers)",
    "ur_attn_plan": "selection query; held by tests/test_attn_plan.py",
    "ur_gemm_plan": "selection query; held by tests/test_gemm_plan.py",
    "ur_lora_plan": "selection query; held by tests/test_lora_plan.py",
    "ur_mean_pool_workspace_bytes": "workspace-size query; one byte less is rejected (test_argument_checks_reject_without_launching)",
    "ur_infonce_workspace_bytes": "workspace-size query; one byte less is rejected (test_argument_checks_reject_without_launching)",
    "ur_heads_workspace_bytes": "workspace-size query",
    "ur_gemm_persistent_mode": "mode switch; both settings are compared bit for bit in tests/test_gpu_gemm_persistent.py",
    "ur_attn_mode": "mode switch; every setting is compared in tests/test_gpu_switches.py",
    "ur_comm_unique_id": "communicator plumbing, no arithmetic; tests/test_gpu_comm.py",
    "ur_comm_init": "communicator plumbing, no arithmetic; tests/test_gpu_comm.py",
    "ur_comm_allreduce_async": "RCCL's sum, not a kernel of this library; tests/test_gpu_comm.py",
    "ur_comm_ticket": "communicator plumbing; tests/test_gpu_comm.py",
    "ur_comm_wait_ticket": "communicator plumbing; tests/test_gpu_comm.py",
    "ur_comm_wait": "communicator plumbing; tests/test_gpu_comm.py",
    "ur_comm_destroy": "communicator plumbing; tests/test_gpu_comm.py",
}


def _headers():
    """include/unirec_hip.h first, then the family headers in name order"""
    first = os.path.join(ROOT, "include", "unirec_hip.h")
    rest = sorted(p for p in glob.glob(os.path.join(ROOT, "include", "unirec_*.h")) if p != first)
    return [first] + rest


def _declared_entry_points():
    """every ur_* function of every header, once: a family header may declare again what it builds on (ur_last_error, ur_catalog_scores,
    ur_catalog_rerank), and a name counts where it first appears"""
    names = []
    for path in _headers():
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        for n in re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", text):
            if n not in names:
                names.append(n)
    return names


def _module(path):
    with open(os.path.join(ROOT, path)) as f:
        return ast.parse(f.read(), filename=path)


@functools.lru_cache(maxsize=None)
def _covers_and_tests(path):
    """(the literal COVERS dict at the top level of the module, the names of its test functions)"""
    tree = _module(path)
    covers = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "COVERS" for t in node.targets):
            covers = ast.literal_eval(node.value)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    return covers, tests


def _problems(declared, tables, tests_of):
    """tables: {module path: COVERS dict}; tests_of(path) -> set of test function names"""
    out = []
    listed = {}
    for path, covers in tables.items():
        for entry, names in covers.items():
            listed.setdefault(entry, []).append(path)
            if entry not in declared:
                out.append(f"{path}: COVERS lists {entry}, which no header under include/ declares")
            if not names:
                out.append(f"{path}: COVERS[{entry!r}] names no test")
            for name in names:
                mod, _, fn = name.rpartition("::")
                mod = mod or path
                if not os.path.exists(os.path.join(ROOT, mod)) or fn not in tests_of(mod):
                    out.append(f"{path}: COVERS[{entry!r}] names {name}, which does not exist")
    for entry in declared:
        if entry in EXEMPT and entry in listed:
            out.append(f"{entry} is both exempt and listed in {listed[entry]}")
        if entry not in EXEMPT and entry not in listed:
            out.append(f"{entry} has no primitive-level test: add one and list it in a COVERS table, or exempt it with a reason")
    for entry in EXEMPT:
        if entry not in declared:
            out.append(f"EXEMPT lists {entry}, which no header under include/ declares")
    return out


def _tables():
    tables = {}
    for path in COVERS_MODULES:
        covers, _ = _covers_and_tests(path)
        assert isinstance(covers, dict), f"{path} has no top-level COVERS dict"
        tables[path] = covers
    return tables


def test_every_entry_point_has_a_primitive_level_test_or_a_reason():
    declared = _declared_entry_points()
    assert len(_headers()) == 11 and len(declared) == len(set(declared))
    assert len(declared) >= 100 and "ur_gemm" in declared and "ur_comm_destroy" in declared
    assert "ur_catalog_deep_select" in declared and "ur_lora_merge" in declared and "ur_catalog_mrl_softmax" in declared
    assert {"ur_catalog_fp8_quantize", "ur_catalog_fp8_select", "ur_catalog_fp8_rerank"} <= set(declared)
    assert all(reason.strip() for reason in EXEMPT.values())
    problems = _problems(declared, _tables(), lambda p: _covers_and_tests(p)[1])
    assert not problems, "\n".join(problems)


def test_the_check_bites():
    """deleting an entry from a COVERS table, naming a test that does not exist, or declaring a new entry point is reported"""
    declared = _declared_entry_points()
    tests_of = lambda p: _covers_and_tests(p)[1]      # noqa: E731
    tables = _tables()
    for path in COVERS_MODULES:
        for entry in tables[path]:
            # (an entry point may be listed by more than one module -- the attention entries are: it is uncovered once EVERY table dropped it)
            cut = {p: {k: v for k, v in c.items() if k != entry} for p, c in tables.items()}
            assert any(entry in msg for msg in _problems(declared, cut, tests_of)), f"deleting {entry} from every table went unnoticed"
            emptied = {p: ({**c, entry: []} if p == path else c) for p, c in tables.items()}
            assert any(entry in msg for msg in _problems(declared, emptied, tests_of)), f"emptying {entry} in {path} went unnoticed"
    renamed = {p: dict(c) for p, c in tables.items()}
    renamed[COVERS_MODULES[1]]["ur_topk"] = ["test_that_was_renamed_away"]
    assert any("test_that_was_renamed_away" in msg for msg in _problems(declared, renamed, tests_of))
    assert any("ur_brand_new_kernel" in msg for msg in _problems(declared + ["ur_brand_new_kernel"], tables, tests_of))
