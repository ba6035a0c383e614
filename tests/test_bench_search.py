"""The driver runs `bench.py` at N=1,2,4,8; its auto plan search must
succeed on every N with the committed measured profiles.  This pins the
CPU-visible part of that path (the search itself — no GPU needed)."""
import pytest

from hetu_galvatron_amd.config import load_config


class _Args:
    model = "llama-3-8b"
    seq_len = 4096
    batch_per_gpu = 8
    chunks = 0
    pp = 1
    tp = 1
    dp_type = "zero2"
    checkpoint = False
    plan = "auto"


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_bench_plan_search_succeeds(world):
    import bench
    args = _Args()
    cfg = load_config(base={
        "model": {"model_name": args.model, "seq_length": args.seq_len},
        "train": {"global_train_batch_size": args.batch_per_gpu * world,
                  "train_iters": 8, "lr": 1e-4,
                  "lr_decay_style": "constant",
                  "distributed_backend": "nccl"},
        "parallel": {"pp_deg": 1, "global_tp_deg": 1,
                     "default_dp_type": "zero2", "chunks": 2,
                     "mixed_precision": "bf16"},
    })
    plan = bench.search_bench_plan(cfg, world, args)
    assert plan is not None, f"bench auto-search found no plan at N={world}"
    assert plan.global_bsz == args.batch_per_gpu * world
    # one full replica per GPU fits in 288 GB: search must not burn the
    # budget on tp/pp/ckpt at bench shapes
    assert plan.pp_deg == 1
    assert all(t == 1 for t in plan.tp_sizes_enc)
    assert not any(plan.checkpoint_flags)
    desc = bench.plan_desc(plan, world)
    assert desc.startswith("searched:")


def _tiny_step():
    """One seeded CPU training step of the tiny preset -> (stats, opt)."""
    import torch
    from hetu_galvatron_amd.runtime import (
        GalvatronModel, get_optimizer_and_param_scheduler, get_train_iterator)
    cfg = load_config(base={
        "model": {"model_name": "tiny-llama"},
        "train": {"global_train_batch_size": 2, "train_iters": 1,
                  "lr": 1e-3, "lr_decay_style": "constant"},
    })
    dev = torch.device("cpu")
    torch.manual_seed(cfg.train.seed)
    model = GalvatronModel(cfg, device=dev)
    opt, sched = get_optimizer_and_param_scheduler(model.stage_model, cfg)
    opt.zero_grad()
    stats = model.forward_backward(next(get_train_iterator(cfg, dev)))
    opt.step()
    sched.step()
    return stats, opt


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float32/float64 .npy files of the last step's loss,
    grad norm and a fixed sample of weights/grads; the same seeded step
    dumps the same arrays (CPU math is deterministic)."""
    import numpy as np
    import bench
    dumps = []
    for name in ("a", "b"):
        stats, opt = _tiny_step()
        out = tmp_path / name
        bench.dump_outputs(str(out), stats, opt)
        dumps.append({p.name: np.load(p) for p in sorted(out.iterdir())})
    a, b = dumps
    assert sorted(a) == ["grad_norm.npy", "grads_sample.npy", "loss.npy",
                         "params_sample.npy"]
    assert a["loss.npy"].dtype == np.float64 and a["loss.npy"].shape == (1,)
    assert a["grad_norm.npy"].dtype == np.float64
    assert a["params_sample.npy"].dtype == np.float32
    assert a["grads_sample.npy"].dtype == np.float32
    assert a["params_sample.npy"].shape == a["grads_sample.npy"].shape
    assert a["params_sample.npy"].size > 0
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert float(a["loss.npy"][0]) == stats.loss
    assert np.abs(a["grads_sample.npy"]).max() > 0
    for k in a:
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k])
