"""CPU tests of the host side: ABI surface, state_dict compatibility with the reference, host logic,
loud failure when the HIP path cannot run, synthetic-data generator stability."""
import os
import re

import numpy as np
import pytest
import torch

from facialmmt_amd import _lib, synth
from facialmmt_amd.config import default_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fmmt_\w+)\s*\(", src)))


def test_header_and_ctypes_signatures_agree():
    assert _header_functions() == sorted(_lib.SIGNATURES)


def test_library_loads_and_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        from facialmmt_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    for name in _header_functions():
        assert hasattr(lib, name), name
    assert lib.fmmt_version() >= 3
    # argument validation happens before any launch, so it is testable without a GPU
    assert lib.fmmt_linear_fwd(1, 10, 96, 95, None, 95, None, 95, None, None, 96, None, 0, None, 96, None, 96, None, 1, None) == -1
    assert lib.fmmt_linear_fwd(7, 10, 96, 96, None, 96, None, 96, None, None, 96, None, 0, None, 96, None, 96, None, 1, None) == -1
    assert lib.fmmt_window_attn_fwd(1, 1, 15, 14, 96, 3, 0, None, None, None, None, 0, 0, 1.0, None, None, None) == -1
    assert lib.fmmt_window_attn_fwd(1, 1, 14, 14, 96, 4, 0, None, None, None, None, 0, 0, 1.0, None, None, None) == -1
    assert lib.fmmt_mha_fwd(1, 8, 8, 1, 500, 4, None, 500, None, None, 500, 1.0, None, 0.0, 0, None, None, 500, None, None) == -1
    assert lib.fmmt_layernorm_fwd(1, 8, 100, None, None, None, 1e-5, None, None, None, 0, None) == -1
    assert lib.fmmt_linear_wgrad_workspace(1, 2007040, 288, 96) > 0
    assert lib.fmmt_linear_wgrad_workspace(0, 125440, 1536, 384) == 256 + 14 * (1536 * 384 + 1536) * 4     # header + fp32 plan's splits
    assert lib.fmmt_window_attn_bwd_workspace(3) == (3 * 257 * 49 * 49 * 4 + 255) // 256 * 256 + 16 * 1024      # d(bias) partials + dense, then the 16 KB store sink (wattn_args.h)


def test_hot_path_refuses_cpu_tensors():
    from facialmmt_amd import ops
    with pytest.raises(_lib.FmmtError, match="GPU only"):
        ops.linear(torch.zeros(4, 96), torch.zeros(96, 96), torch.zeros(96))
    with pytest.raises(_lib.FmmtError):
        ops.layer_norm(torch.zeros(4, 96), torch.ones(96), torch.zeros(96))


def test_state_dict_keys_match_reference(golden):
    from facialmmt_amd import models
    from facialmmt_amd.modules.CrossmodalTransformer import CrossModalTransformerEncoder
    from facialmmt_amd.modules.multihead_attention import MultiheadAttention
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as S

    def keys(m):
        return [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()]
    args = default_args()
    aff = models.SwinForAffwildClassification(args)
    assert keys(aff) == golden.keys["affwild"]
    assert keys(aff.swin) == golden.keys["swin"]
    assert keys(CrossModalTransformerEncoder(768, 12, 2, 0.1)) == golden.keys["crossmodal"]
    assert keys(CrossModalTransformerEncoder(500, 4, 2, 0, 0, 0, 0)) == golden.keys["enc500"]
    assert keys(MultiheadAttention(768, 12, attn_dropout=0.1)) == golden.keys["mha"]
    assert keys(S.SwinTransformerBlock(96, (56, 56), 3, shift_size=3)) == golden.keys["blk0_shift3"]
    assert keys(S.SwinTransformerBlock(768, (7, 7), 24, shift_size=3)) == golden.keys["blk3_shift3"]   # shift forced to 0: no mask entry
    assert keys(S.PatchMerging((56, 56), 96)) == golden.keys["pm0"]
    assert keys(S.PatchEmbed(224, 4, 3, 96, torch.nn.LayerNorm)) == golden.keys["pe"]
    for plm in ("roberta", "bert"):
        cfg = default_args(get_audio_utt_max_lens=24, get_vision_utt_max_lens=20,
                           pretrainedtextmodel_path=f"pretrained_model/{plm}-large", plm_module=synth.make_standin_plm())
        assert keys(models.MultiModalTransformerForClassification(cfg)) == golden.keys["multimodal_" + plm]
    assert keys(models.meld_utt_transformer(default_args(get_vision_utt_max_lens=20))) == golden.keys["meld_utt"]


def test_structural_buffers_match_oracle():
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as S
    from oracle import swin as OS
    for H in (56, 28, 14):
        assert torch.equal(S.build_shift_mask(H, H, 7, 3), OS.shift_mask(H, H, 7, 3))
    assert torch.equal(S.WindowAttention(96, (7, 7), 3).relative_position_index, OS.relative_position_index(7))
    blk = S.SwinTransformerBlock(768, (7, 7), 24, shift_size=3)
    assert blk.shift_size == 0 and blk.attn_mask is None


def test_reference_asserts_are_kept():
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as S
    with pytest.raises(AssertionError, match="doesn't match model"):
        S.PatchEmbed(224, 4, 3, 96)(torch.zeros(1, 3, 112, 112))
    with pytest.raises(AssertionError, match="wrong size"):
        S.SwinTransformerBlock(96, (56, 56), 3)(torch.zeros(1, 100, 96))
    with pytest.raises(AssertionError, match="not even"):
        S.PatchMerging((7, 7), 768)(torch.zeros(1, 49, 768))
    with pytest.raises(NotImplementedError):
        S.WindowAttention(96, (8, 8), 3).cuda if False else S.WindowAttention(96, (8, 8), 3)._check()


def test_slice_target_utterance_matches_literal_loop():
    from facialmmt_amd.models import slice_target_utterance
    from oracle.multimodal import slice_target_utterance_loop
    g = torch.Generator().manual_seed(0)
    for trial in range(20):
        B, T, H = 5, 60, 8
        feats = torch.randn(B, T, H, generator=g)
        sep = torch.zeros(B, T)
        for i in range(B):                      # separators at least 3 tokens apart (closer ones make the reference itself raise)
            pos = 1
            while True:
                pos += int(torch.randint(3, 14, (1,), generator=g))
                if pos >= T:
                    break
                sep[i, pos] = 1
        utt = torch.randint(0, 5, (B,), generator=g)
        for roberta in (True, False):
            a, am = slice_target_utterance(feats, sep, utt, 7, roberta)
            b, bm = slice_target_utterance_loop(feats, sep, utt, 7, roberta)
            assert torch.equal(a, b) and torch.equal(am, bm)


def test_positional_embedding_module_matches_oracle(golden):
    from facialmmt_amd.modules.position_embedding import SinusoidalPositionalEmbedding
    pin = torch.from_numpy(golden.files["crossmodal"]["posemb/in"])
    golden.check("crossmodal", "posemb/out", SinusoidalPositionalEmbedding(768)(pin), atol=1e-6, rtol=1e-6)


def test_droppath_scale_statistics():
    from facialmmt_amd.modules.SwinTransformer.Swin_Transformer import DropPath
    torch.manual_seed(0)
    dp = DropPath(0.3).train()
    s = dp.sample_scale(20000, "cpu")
    assert [round(float(v), 4) for v in s.unique()] == [0.0, round(1 / 0.7, 4)]
    assert abs(s.mean().item() - 1.0) < 0.02
    assert DropPath(0.3).eval().sample_scale(8, "cpu") is None


def test_synth_is_stable():
    """the generator is the contract between the committed goldens and the GPU box: pin a few values"""
    u = synth.uniform("frames", (4,), seed=1)
    assert u.dtype == np.float32
    assert np.allclose(u, synth.uniform("frames", (2, 2), seed=1).reshape(-1))
    assert np.array_equal(synth.uniform("frames", (1000,), seed=1)[:4], u)
    assert synth.uniform("a", (3,), 0).tolist() != synth.uniform("b", (3,), 0).tolist()
    assert synth.randint("x", (100,), 3, 10).min() >= 3 and synth.randint("x", (100,), 3, 10).max() < 10


def test_swin_mac_formula_matches_survey():
    from oracle.swin import swin_macs_per_frame
    m = swin_macs_per_frame()
    assert abs(m["total"] / 1e9 - 4.5128) < 2e-3 and abs(m["stage0"] / 1e6 - 811.9) < 0.2 and abs(m["head"] / 1e6 - 19.27) < 0.01


def test_shadow_cache_is_per_parameter_object_not_per_address():
    """ops._lp: a new parameter that lands on the memory (and version count) of a dead one must not be served the dead
    one's cached shadow; views of one parameter (in_proj_weight[a:b]) share the parameter's cache and see its updates."""
    import gc
    from facialmmt_amd import ops
    def make(val):
        p = torch.nn.Parameter(torch.full((8, 16), val))
        return p
    p = make(1.0)
    t1 = ops._lp(p, torch.float32, transpose=True)
    assert t1.shape == (16, 8) and float(t1[0, 0]) == 1.0
    assert ops._lp(p, torch.float32, transpose=True) is t1                       # cached
    key = id(p)
    assert key in ops._CAST_CACHE
    del p, t1
    gc.collect()
    assert key not in ops._CAST_CACHE                                            # dropped with the parameter
    q = make(2.0)
    assert float(ops._lp(q, torch.float32, transpose=True)[0, 0]) == 2.0
    v = ops._lp(q[2:6], torch.bfloat16)
    assert v.shape == (4, 16) and v.dtype == torch.bfloat16 and ops._lp(q[2:6], torch.bfloat16) is v
    with torch.no_grad():
        q.mul_(3.0)                                                              # optimizer step: version bump
    assert float(ops._lp(q[2:6], torch.bfloat16)[0, 0]) == 6.0


def test_checkpoint_backbone_mapping_and_round_trip(tmp_path):
    """FaceX-Zoo `backbone.` mapping (train.py:316-331) and plain state_dict files."""
    from facialmmt_amd import checkpoint, models
    torch.manual_seed(3)
    m = models.SwinForAffwildClassification(default_args())
    own = m.state_dict()
    # a FaceX-Zoo style file: backbone.<name> for the Swin, its own head.*, and a classifier of another width
    file_sd = {}
    for k, v in own.items():
        if k.startswith("swin."):
            file_sd["backbone." + k[5:]] = torch.full_like(v, 0.5) if v.is_floating_point() else v.clone()
    file_sd["head.weight"] = torch.zeros(93431, 512)[:4]
    file_sd["backbone.classifier.weight"] = torch.ones_like(own["classifier.weight"])
    path = tmp_path / "Swin_tiny_Ms-Celeb-1M.pt"
    torch.save({"state_dict": file_sd, "epoch": 17}, path)
    rep = checkpoint.load_pretrained_backbone(m, str(path))
    after = m.state_dict()
    swin_keys = [k for k in own if k.startswith("swin.")]
    assert sorted(rep.loaded) == sorted(swin_keys) and not rep.mismatched
    assert sorted(rep.missing) == sorted(k for k in own if not k.startswith("swin.") and not k.startswith("classifier."))
    assert "head.weight" in rep.unused and "backbone.classifier.weight" in rep.unused
    for k in swin_keys:
        if own[k].is_floating_point():
            assert bool((after[k] == 0.5).all()), k
    for k in own:
        if not k.startswith("swin."):
            assert torch.equal(after[k], own[k]), k         # head keeps its initial values; classifier never loaded

    # wrapped training-time module -> plain file -> fresh model, exact
    wrapped = torch.nn.Sequential()
    wrapped.add_module("module", m)                          # keys become "module.<name>" like DataParallel / _LiteModule
    sd = checkpoint.extract_state_dict(wrapped)
    assert list(sd) == list(own)
    out = tmp_path / "best_swin.pt"
    checkpoint.save_state(wrapped, str(out), extra={"best_f1": 0.66})
    raw = torch.load(out, weights_only=True)
    assert raw["best_f1"] == 0.66 and list(raw["state_dict"]) == list(own)
    m2 = models.SwinForAffwildClassification(default_args())
    rep2 = checkpoint.load_state(m2, str(out))
    assert not rep2.missing and not rep2.unused and not rep2.mismatched
    for k, v in m2.state_dict().items():
        assert torch.equal(v, after[k]), k
    # strict load refuses a file that does not fit
    bad = dict(sd)
    bad.pop("linear.weight")
    with pytest.raises(RuntimeError, match="missing"):
        checkpoint.load_state(m2, bad)
    rep3 = checkpoint.load_state(m2, bad, strict=False)
    assert rep3.missing == ["linear.weight"]
    with pytest.raises(KeyError):
        checkpoint.extract_state_dict({"module.a": torch.zeros(1), "a": torch.zeros(1)})


def test_convert_checkpoint_unwraps_whole_module_pickles(tmp_path):
    """tools/convert_checkpoint.py: a whole-module pickle (utils/util.py:121-133) wrapped as LightningLite / DataParallel
    wrap it -> a plain file that torch.load(weights_only=True) reads, with the wrapper prefixes gone."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import convert_checkpoint
    from facialmmt_amd import checkpoint
    from tests.pickle_fixture import TinyHead, _LiteModule
    torch.manual_seed(0)
    inner = TinyHead()
    src, out = str(tmp_path / "multimodal_model_T+A+V_x.pt"), str(tmp_path / "plain.pt")
    torch.save(_LiteModule(torch.nn.DataParallel(inner)), src, pickle_protocol=4)
    rep = convert_checkpoint.convert(src, out, reference_root=str(tmp_path), expect_class="TinyHead")
    assert rep["wrappers"] == ["_LiteModule", "DataParallel"] and rep["n_tensors"] == len(inner.state_dict())
    payload = torch.load(out, weights_only=True)
    assert list(payload["state_dict"]) == list(inner.state_dict()) and payload["class"] == "TinyHead"
    fresh = TinyHead()
    checkpoint.load_state(fresh, out)
    for k, v in inner.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v.cpu()), k          # DataParallel moved `inner` to cuda:0 where a GPU is visible
    with pytest.raises(TypeError, match="expected"):
        convert_checkpoint.convert(src, out, expect_class="SwinForAffwildClassification")
    assert convert_checkpoint.main(["--in", src, "--out", out]) == 0


def test_plm_pooler_is_kept_but_frozen():
    """the PLM pooler never receives a gradient (forward reads last_hidden_state only); it keeps its
    state_dict keys but must not be a trainable parameter a data-parallel exchange would wait for."""
    from transformers import RobertaConfig
    from facialmmt_amd import models
    cfg = default_args()
    cfg.plm_config = RobertaConfig(vocab_size=100, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                   max_position_embeddings=40, type_vocab_size=1, pad_token_id=1)
    mm = models.MultiModalTransformerForClassification(cfg)
    assert "roberta.pooler.dense.weight" in mm.state_dict()
    assert all(not p.requires_grad for p in mm.roberta.pooler.parameters())
    assert all(p.requires_grad for n, p in mm.named_parameters() if ".pooler." not in n)


def test_bench_contract_flags_and_loud_failure_without_gpu():
    """bench.py keeps the driver's flag contract and, like the rest of the product path, refuses to run without
    the GPU instead of falling back to anything (the CPU baseline leg is only ever timed beside the HIP path)."""
    import subprocess
    import sys
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, env=env, timeout=300)
    assert h.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in h.stdout
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible to this process")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr
    assert not r.stdout.strip().startswith("{")            # no metric line from a run that measured nothing


def test_bench_gpus_n_runs_as_typed():
    """`python bench.py --gpus 2` with no launcher around it (WORLD_SIZE unset) runs itself under torch.distributed.run as a child, one rank per
    GPU on 127.0.0.1, instead of dying on an assertion (round-5 VERDICT item 6).  --rendezvous-check stops behind the process group (gloo
    here: no GPU), rank 0 prints the one JSON line with the number of ranks the all-reduce saw."""
    import json
    import subprocess
    import sys
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.spawn_command(["--gpus", "8", "--steps", "3"], 8, port=29555)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"] and cmd[-5].endswith("bench.py")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(FMMT_BENCH_BACKEND="gloo", FMMT_BENCH_DEVICE="0", FMMT_BENCH_PORT=str(29600 + os.getpid() % 300))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rendezvous-check"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["rendezvous_check"] is True and line["ranks_seen"] == 2 and line["world_size"] == 2 and line["n_gpus"] == 2
    # a launcher whose --nproc-per-node disagrees with --gpus is still refused
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rendezvous-check"], capture_output=True, text=True, env=env2, timeout=300)
    assert r2.returncode != 0 and "--nproc-per-node must equal --gpus" in r2.stderr


def test_capture_window_fences_the_cyclic_collector():
    """train_step.capture_window: collect before a graph capture, collector off inside, previous state restored after
    (also when the body raises, and when the collector was already off)."""
    import gc
    from facialmmt_amd.train_step import capture_window

    class Node:
        pass
    a, b = Node(), Node()
    a.other, b.other = b, a
    import weakref
    seen = weakref.ref(a)
    del a, b
    assert gc.isenabled()
    with capture_window():
        assert seen() is None and not gc.isenabled()
    assert gc.isenabled()
    with pytest.raises(ValueError):
        with capture_window():
            raise ValueError("x")
    assert gc.isenabled()
    gc.disable()
    try:
        with capture_window():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()


def test_master_weights_keep_frozen_parameters_and_buffers_in_fp32():
    """MasterWeights turns a module to bf16 in place; its checkpoint view (state_dict_fp32) must hold the fp32 masters of the stepped
    parameters AND the untouched fp32 values of what has no master: frozen parameters (the text encoder's unused pooler) and buffers."""
    import torch
    from facialmmt_amd.train_step import MasterWeights
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(24, 16), torch.nn.LayerNorm(16), torch.nn.Linear(16, 8))
    m.register_buffer("stat", torch.randn(5) * 1.2345678)
    for p in m[2].parameters():
        p.requires_grad_(False)                              # a frozen tail, like the pooler
    want = {k: v.detach().clone() for k, v in m.state_dict().items()}
    mw = MasterWeights(m, torch.bfloat16)
    assert all(p.dtype == torch.bfloat16 for p in m.parameters())
    got = mw.state_dict_fp32()
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and torch.equal(got[k], v), k


def test_hf_adamw_state_dict_round_trip_keeps_the_lr_tensor_and_continues_the_run():
    """HFAdamW.hf_state_dict -> load_hf_state_dict (the transformers.AdamW layout of the reference's checkpoints, train.py:316-331: float lr, an
    int step per parameter): the group's lr TENSOR object survives (the graphed steps and the scheduler address it) filled with the
    saved value, the step counter continues, and the next step equals the uninterrupted run's."""
    from facialmmt_amd.train_step import HFAdamW
    g = torch.Generator().manual_seed(3)
    shapes = [(17, 5), (9,)]
    init = [torch.randn(sh, generator=g) for sh in shapes]
    a = [torch.nn.Parameter(t.clone()) for t in init]
    opt_a = HFAdamW(a, lr=torch.tensor(3e-3), weight_decay=0.01)
    grads = [[torch.randn(sh, generator=g) for sh in shapes] for _ in range(4)]
    for k in range(3):
        for p, gr in zip(a, grads[k]):
            p.grad = gr.clone()
        opt_a.step()
    import copy
    sd = copy.deepcopy(opt_a.hf_state_dict())               # (as read from a file: Optimizer.load_state_dict does not copy same-dtype tensors)
    sd["param_groups"][0]["lr"] = 2e-3                       # as transformers.AdamW stores it: a Python float (here: another value than the live one)
    assert all(sd["state"][i]["step"] == 3 for i in sd["state"]) and "step" not in sd["param_groups"][0]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    lr_b = torch.tensor(7e-3)
    opt_b = HFAdamW(b, lr=lr_b, weight_decay=0.01)
    for p, gr in zip(b, grads[0]):                           # a live optimizer: state and counter exist already
        p.grad = gr.clone()
    opt_b.step()
    with torch.no_grad():
        for p, q in zip(b, a):
            p.copy_(q)
    step_b = opt_b.param_groups[0]["step"]
    opt_b.load_hf_state_dict(sd)
    gb = opt_b.param_groups[0]
    assert gb["lr"] is lr_b and abs(float(lr_b) - 2e-3) < 1e-9          # same tensor object, saved value
    assert gb["step"] is step_b and float(step_b) == 3.0
    assert gb["correct_bias"] is True and gb["eps"] == 1e-6
    opt_a.param_groups[0]["lr"].fill_(2e-3)
    for pa, pb, gr in zip(a, b, grads[3]):
        pa.grad = gr.clone()
        pb.grad = gr.clone()
    opt_a.step()
    opt_b.step()
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)
    assert float(gb["step"]) == 4.0
    bad = opt_a.hf_state_dict()
    bad["state"][0]["step"] = 1
    with pytest.raises(ValueError):
        opt_b.load_hf_state_dict(bad)
