#!/usr/bin/env python3
"""The parameter EMA under data parallel, on a one-GPU box (run under torchrun, ONE rank):

    python -m torch.distributed.run --nproc-per-node 1 --master-addr 127.0.0.1 --master-port P \
        tools/ema_dp_check.py [--steps 3] [--precision bf16x3] [--decay 0.999]

The rank creates the production process group and trains K phased TrainSteps with ema_decay set and
GradSync forced to issue both all-reduce buckets at world 1 (tools/rccl_check.py has the details). The
EMA issues no collective: every rank averages identical parameters with a deterministic kernel, so
`ema`, the parameters and n_averaged must equal, bit for bit, those of the same phased steps without a
process-group collective. Prints one JSON line; exit 1 on a mismatch.
"""
import argparse
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def train(dev, precision, steps, batch, decay, force_sync):
    import fall_multimodal_amd as f3
    from oracle.prng import synthetic_batch
    torch.manual_seed(0)
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=dev,
                                      precision=precision)
    step = f3.TrainStep(model, batch, lr=1e-3, phased=True, force_sync=force_sync, ema_decay=decay)
    for i in range(steps):
        step(*[torch.from_numpy(x).to(dev) for x in synthetic_batch(batch, 18, 11, 6, 500 + i)])
    torch.cuda.synchronize()
    return model.flat_parameters().clone(), step.ema.clone(), int(step.n_averaged.item()), step.sync


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--decay", type=float, default=0.999)
    a = ap.parse_args()
    assert int(os.environ["WORLD_SIZE"]) == 1, "one rank: the one-GPU check"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from fall_multimodal_amd.train import rccl_options
    dist.init_process_group("nccl", pg_options=rccl_options())
    p_dp, e_dp, n_dp, sync = train(dev, a.precision, a.steps, a.batch, a.decay, True)
    p_ref, e_ref, n_ref, _ = train(dev, a.precision, a.steps, a.batch, a.decay, False)
    i32 = torch.int32
    res = {"world": dist.get_world_size(), "steps": a.steps, "precision": a.precision, "decay": a.decay,
           "grad_sync_active": sync.active, "n_averaged": [n_dp, n_ref],
           "ema_bit_identical": bool(torch.equal(e_dp.view(i32), e_ref.view(i32))),
           "params_bit_identical": bool(torch.equal(p_dp.view(i32), p_ref.view(i32))),
           "ema_lags_params": not bool(torch.equal(e_dp.view(i32), p_dp.view(i32)))}
    print(json.dumps(res), flush=True)
    dist.destroy_process_group()
    ok = (res["ema_bit_identical"] and res["params_bit_identical"] and res["grad_sync_active"]
          and res["ema_lags_params"] and n_dp == n_ref == a.steps)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
