"""Child process of tests/test_gpu_distributed.py: one data-parallel rank on cuda:0 (gloo rendezvous on 127.0.0.1) with the REAL engine.
argv: rank world port steps out_path [backend [payload [draw|explicit [shards]]]]; shards: per-step shard sizes of every rank, steps
separated by ":" and ranks by "," ("32,32:24,16": a global batch of 64 split 32 / 32, then one of 40 split 24 / 16)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(dev, B, T=200):
    """Model, binding and the WHOLE synthetic batch (every rank builds the same one and takes its shard)."""
    from structured_latent_odes_amd.configs import load_config_cvs
    from structured_latent_odes_amd.models.mechanistic_cvs import MechanisticModel
    from structured_latent_odes_amd.synthetic import synthetic_batch
    from structured_latent_odes_amd.utils.utils import set_seed
    cfg = load_config_cvs()
    cfg.update(seq_len=T, z_iext_dim=3, z_rtpr_dim=3, z_epsilon_dim=2, solver="rk4", mini_batch_size=B)
    set_seed(cfg.seed)
    times = torch.arange(0.0, T * cfg.delta_t, cfg.delta_t, device=dev)
    model = MechanisticModel(cfg, dev, times)
    obs, labels, _ = synthetic_batch("cvs", B, T, 3, seed=4321)
    u = model.labels_to_u(**{k: v.to(dev) for k, v in labels.items()})
    eps = torch.randn(B, model.latent_dim, generator=torch.Generator().manual_seed(7)).to(dev)
    return cfg, model, obs.to(dev), u, eps


def run(rank, world, steps, B=64, payload="G", unfused=False, draw=False, shards=None):
    """shards: per-step list of every rank's shard size (``parse_shards``); global batch k is the next sum(shards[k]) rows of one
    synthetic batch and rank r takes the rows after the shards of the lower ranks (``steps`` and ``B`` are then implied; without it
    every step takes the same batch of B, split evenly);
    payload: what the data-parallel step all-reduces ("G": [G | head products | ODE-half row], "grad": [flat gradient | loss]);
    unfused: take the data-parallel code path at world size 1 too; draw: noise drawn in the kernels (keyed by the GLOBAL trajectory index,
    so the sharded run and the whole-batch run see the same noise) instead of the explicit eps tensor."""
    from structured_latent_odes_amd.svi import ELBOStep, FlatAdam
    dev = torch.device("cuda", 0)
    if shards is None:                                   # the same batch of B in every step, split evenly
        plan = [(0, [B // world] * world)] * steps
    else:
        starts = [sum(sum(s) for s in shards[:k]) for k in range(len(shards))]
        plan, B = list(zip(starts, shards)), sum(sum(s) for s in shards)
    cfg, model, obs, u, eps = build(dev, B)
    b = model._bind()
    b.engine.rng_seed(2026)
    svi = ELBOStep(b.engine, b.flat, FlatAdam(b.engine, b.flat, lr=cfg.learning_rate))
    svi.dp_payload, svi.unfused = payload, unfused
    assert svi.world == world
    losses = []
    for start, sizes in plan:
        assert len(sizes) == world, (sizes, world)
        lo = start + sum(sizes[:rank])
        sl = slice(lo, lo + sizes[rank])
        e = None if draw else eps[sl].contiguous()
        losses.append(float(svi.step(obs[sl], eps=e, u=u[sl].contiguous())))
    e = None if draw else eps[sl].contiguous()
    ev = svi.evaluate_loss(obs[sl], eps=e, u=u[sl].contiguous())     # the last global batch again (a drawing call of its own)
    res = dict(losses=losses, eval_loss=ev, params=b.flat.detach().cpu().clone(), grads=svi.grads.detach().cpu().clone(),
               collective_bytes=svi.collective_bytes)
    if torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl":
        res["nccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    return res


def parse_shards(text):
    return [[int(v) for v in step.split(",")] for step in text.split(":")] if text else None


if __name__ == "__main__":
    rank, world, port, steps, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), sys.argv[5]
    backend = sys.argv[6] if len(sys.argv) > 6 else "gloo"
    payload = sys.argv[7] if len(sys.argv) > 7 else "G"
    draw = len(sys.argv) > 8 and sys.argv[8] == "draw"
    shards = parse_shards(sys.argv[9]) if len(sys.argv) > 9 else None
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    if backend == "nccl":
        torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))   # as bench.py does
    else:
        torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    res = run(rank, world, steps, payload=payload, unfused=(world == 1), draw=draw, shards=shards)
    if rank == 0:
        torch.save(res, out)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
