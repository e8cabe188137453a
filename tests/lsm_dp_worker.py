"""Worker of tests/test_resample_gpu.py::test_two_ranks_hold_one_history: one data-parallel rank of HotPathTrainer.step with a
LossSecondMomentResampler, on the tiny learned-variance UNet.  Launched by `python -m torch.distributed.run --nproc-per-node 2`; both
ranks use the ONE visible GPU, collectives over gloo (as tests/dp_worker.py).  Every rank records the (index, loss) rows it hands to the
history update; rank 0 writes every rank's rows and final hist / count / pos to --out."""
import argparse
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd")]

T, K, B = 8, 2, 3


def run(rank, world, steps, dev="cuda"):
    import v_diffusion as vd
    from v_diffusion.trainer import HotPathTrainer
    from oracle.cases import TINY, make_inputs, make_weights
    case = TINY["tinyA"]
    cfg = dict(case["cfg"], out_channels=6)
    model = vd.UNet(**cfg)
    model.load_state_dict(make_weights(cfg), strict=True)
    model.to(dev).train()
    gd = vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), T, "v", "learned", "snr_trunc", "kl", w_guide=0.0, p_uncond=0.0)
    tr = HotPathTrainer(model, gd, lr=1e-3, warmup=0, timesteps=T, rank=rank, world_size=world,
                        schedule_sampler=vd.LossSecondMomentResampler(T, history_per_term=K, device=dev))
    reported = []
    inner = tr._update_history

    def recording(idx, per):
        reported.append((idx.detach().cpu().clone(), per.detach().cpu().clone()))
        inner(idx, per)
    tr._update_history = recording
    for s in range(steps):
        x0, _, y = make_inputs(case["cfg"], B, case["R"], case["label"], seed=41 + 2 * s + rank)
        x0 = (x0.clamp(-1, 1) * 127.5).round() / 127.5
        tr.step(x0.to(dev), y.clamp(min=1).to(dev))
    torch.cuda.synchronize()
    sm = tr.sampler
    return dict(rows=reported, hist=sm.hist.cpu(), count=sm.count.cpu(), pos=sm.pos.cpu())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=2)
    a = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = run(rank, world, a.steps)
    every = [None] * world
    dist.all_gather_object(every, res)
    if rank == 0:
        torch.save(dict(ranks=every, T=T, K=K, B=B), a.out)
    dist.destroy_process_group()
