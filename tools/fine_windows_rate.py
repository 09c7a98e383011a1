"""Wall time of MusicLM.generate(return_tokens=True, output_seconds=10) with the fine windows one after the other and together
(fine_windows_together), on depth-6 dim-1024 stages: whole call and the fine stage alone (host clock around device synchronises).
The comparison is between two settings of ONE build.  env: PROMPTS (1), PREC (fp16ff), REPS (3)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import open_musiclm as M

dev = torch.device("cuda:0")
P = int(os.environ.get("PROMPTS", 1)); prec = os.environ.get("PREC", "fp16ff"); reps = int(os.environ.get("REPS", 3))
torch.manual_seed(0)
kw = dict(dim=1024, depth=6, heads=8, precision=prec)
mlm = M.MusicLM(wav2vec=None, clap=None, neural_codec=None, semantic_transformer=M.create_semantic_transformer(**kw).to(dev),
                coarse_transformer=M.create_coarse_transformer(num_coarse_quantizers=3, **kw).to(dev),
                fine_transformer=M.create_fine_transformer(num_coarse_quantizers=3, num_fine_quantizers=5, **kw).to(dev))
clap_ids = torch.randint(0, 1024, (P, 12, 1), generator=torch.Generator().manual_seed(5)).to(dev)
fine_s = [0.0]
orig = mlm.fine.generate


def timed_fine(*a, **k):
    torch.cuda.synchronize(); t = time.perf_counter()
    out = orig(*a, **k)
    torch.cuda.synchronize()
    fine_s[0] += time.perf_counter() - t
    return out


mlm.fine.generate = timed_fine


def run(together):
    fine_s[0] = 0.0
    torch.manual_seed(1)
    torch.cuda.synchronize(); t = time.perf_counter()
    s, c, f = mlm.generate(clap_token_ids=clap_ids, output_seconds=10, return_tokens=True, fine_windows_together=together)
    torch.cuda.synchronize()
    return time.perf_counter() - t, fine_s[0], tuple(f.shape)


for together in (False, True):
    run(together)                                               # warm-up of every shape the timed calls use
for rep in range(reps):
    for together in (False, True):                              # alternating
        total, fine, shape = run(together)
        print(f"prompts={P} {prec} fine_windows_together={together} rep={rep}: whole call {total:.3f} s, fine stage {fine:.3f} s, fine ids {shape}",
              flush=True)
