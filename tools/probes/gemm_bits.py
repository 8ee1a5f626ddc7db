"""Development aid: are two builds of the library the same function?  Seeded operands through every epilogue of ops.linear_raw and every form of
ops.wgrad_raw at the shapes of nt_probe.py, tn_probe.py, few_probe.py and one shape per remaining arm of the dispatch; one integer checksum (int64 sum of
the outputs' raw 16- / 32-bit words) per case.  Run once per library (PROBE_LIB), diff the two outputs: they must be textually identical."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from facialmmt_amd import _lib
if os.environ.get("PROBE_LIB"):                                # A/B of two builds in one call
    _lib.LIB_PATH = os.environ["PROBE_LIB"]
from facialmmt_amd import ops
from facialmmt_amd._lib import EPI_GELU, EPI_GELU_BWD, EPI_GELU_DG, EPI_MUL_AUX
dev = torch.device("cuda:0")
bf, f32 = torch.bfloat16, torch.float32
NT = [(501760, 576, 192), (501760, 768, 192), (501760, 192, 768), (125440, 1152, 384), (125440, 1536, 384), (125440, 384, 384),      # nt_probe.py
      (125440, 384, 1536), (125440, 384, 1152), (31360, 2304, 768), (31360, 3072, 768), (31360, 768, 3072), (31360, 768, 768)]
TN = [(125440, 384, 768), (31360, 768, 1536)]                                                                                        # tn_probe.py (what NT lacks)
FEW = [(152, 768, 768), (166, 768, 768), (512, 768, 768), (640, 768, 768), (1328, 768, 768), (664, 1536, 768), (512, 2304, 768),     # few_probe.py
       (512, 3072, 768), (512, 768, 3072), (1328, 3072, 768), (1328, 768, 3072), (640, 512, 768), (600, 768, 768)]
ARMS = [(65613, 384, 96), (70000, 288, 96), (20000, 384, 96), (3000, 96, 96),       # K = 96: unrolled deep kernels (128- / 96-wide), single-step 128- / 64-row tiles
        (50176, 96, 48), (6272, 96, 48),                                            # K = 48 (PatchEmbed)
        (640, 512, 37632), (640, 37632, 512),                                       # embedding head: split-K forward; its input gradient (128-row tiles, few rows)
        (65600, 96, 384), (70000, 576, 192), (65536, 96, 288),                      # deep, N % 96
        (65613, 384, 1536), (65613, 128, 768), (65613, 384, 384),                   # deep, ragged M: K step 64 (plain, K > 512) / K step 32
        (20008, 1536, 384), (7840, 1536, 1536), (4104, 2304, 768), (5000, 200, 72)] # persistent kernel with a ragged panel; phase kernels; register-staged K step 32 (K % 64 != 0)
F32 = [(500, 96, 96), (3000, 384, 96), (5000, 96, 384), (8200, 128, 256)]           # fp32 parity path


def words(t):
    return int(t.view(torch.int16 if t.dtype == bf else torch.int32).to(torch.int64).sum().item())


ncase = 0
def out(tag, M, N, K, dt, *ts):
    global ncase
    ncase += 1
    print(f"{tag:22s} {str(dt)[6:]:8s} {M:7d}x{N:5d}x{K:5d} " + " ".join(str(words(t)) for t in ts if t is not None), flush=True)


for dt, shapes in ((bf, NT + TN + FEW + ARMS), (f32, F32)):
    for (M, N, K) in shapes:
        g = torch.Generator(device=dev)
        g.manual_seed(M * 7 + N * 3 + K)
        rnd = lambda *s, dtype=dt: torch.randn(*s, device=dev, dtype=torch.float32, generator=g).to(dtype)
        x, w, b = rnd(M, K), rnd(N, K) * K ** -0.5, rnd(N, dtype=f32)
        aux, res = rnd(M, N), rnd(M, N)
        rps = 196 if M % 196 == 0 else (49 if M % 49 == 0 else 64)
        ns = (M + rps - 1) // rps
        rs = rnd(ns, dtype=f32).abs() + 0.5                    # a general scale vector for the forward ...
        drop = torch.full((ns,), 1.0 / 0.9, device=dev)        # ... DropPath's two-valued one, a sample dropped, for the weight gradient
        drop[1 % ns::10] = 0.0
        a = (M, N, K, dt)
        out("linear plain", *a, ops.linear_raw(x, w, None))
        out("linear bias", *a, ops.linear_raw(x, w, b))
        pre = torch.zeros(M, N, device=dev, dtype=dt)
        out("linear gelu+pre", *a, ops.linear_raw(x, w, b, epi=EPI_GELU, y_pre=pre), pre)
        pre.zero_()
        out("linear gelu_dg", *a, ops.linear_raw(x, w, b, epi=EPI_GELU_DG, y_pre=pre), pre)
        out("linear mul_aux", *a, ops.linear_raw(x, w, None, epi=EPI_MUL_AUX, aux=aux))
        out("linear mul_aux+scale", *a, ops.linear_raw(x, w, None, epi=EPI_MUL_AUX, aux=aux, rowscale=rs, rows_per_scale=rps))
        out("linear gelu'", *a, ops.linear_raw(x, w, None, epi=EPI_GELU_BWD, aux=aux))
        out("linear res+scale", *a, ops.linear_raw(x, w, b, res=res, rowscale=rs, rows_per_scale=rps))
        out("linear scale", *a, ops.linear_raw(x, w, None, rowscale=rs, rows_per_scale=rps))
        del pre, res
        dy = aux                                               # [M][N]
        out("wgrad plain", *a, ops.wgrad_raw(dy, x, False)[0])
        out("wgrad bias", *a, *ops.wgrad_raw(dy, x, True))
        out("wgrad dropped sample", *a, *ops.wgrad_raw(dy, x, True, drop, rps))
        out("wgrad x_gelu", *a, *ops.wgrad_raw(dy, x, True, x_gelu=True))
        del x, w, aux, dy
torch.cuda.synchronize()
print(f"cases {ncase}")
