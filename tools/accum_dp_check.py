#!/usr/bin/env python3
"""Data-parallel check of the accumulating training step (run under torchrun, as tools/dp_check.py):

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P \
        tools/accum_dp_check.py [--backend gloo] [--same-device]

Each rank runs five batches of its own synthetic shard through TrainStep(accum_iter=3) after
begin_epoch(5): updates are due after batches 0, 3 and 4 (the reference's rule, model/main.py:115-132).
Reported as one JSON line by rank 0:
* all_reduce_rounds: rounds of the two-bucket all-reduce issued by the five calls (3: the calls that
  do not update issue no collective), all_reduce_calls the collectives themselves (2 per round);
* window_sum_bitwise: after the first window of three micro-batches (batches 1-3) the reduced `accum`
  equals local accum of rank 0 + local accum of rank 1 bit for bit (a two-term fp32 sum has one order);
* replicas_identical: every rank ends with bit-identical parameters, which moved.
"""
import argparse
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="nccl")
    ap.add_argument("--same-device", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = 0 if a.same_device else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if a.backend == "nccl":
        from fall_multimodal_amd.train import rccl_options
        dist.init_process_group(a.backend, pg_options=rccl_options())
    else:
        dist.init_process_group(a.backend)
    dev = torch.device("cuda", local)
    import fall_multimodal_amd as f3
    from fall_multimodal_amd.train import accum_updates
    from oracle.prng import synthetic_batch
    torch.manual_seed(0)  # identical init on every rank
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, 11, 6, device=dev,
                                      precision=a.precision)
    p0 = model.flat_parameters().clone()
    step = f3.TrainStep(model, a.batch, lr=1e-3, accum_iter=3)
    assert step.world == world and step.sync.active

    counts = {"rounds": 0, "calls": 0, "on": False}
    local_accum = []  # this rank's accum as each round's all-reduce found it
    real_all, real_reduce = step.sync.all, dist.all_reduce

    def counted_reduce(*args, **kw):
        if counts["on"]:
            counts["calls"] += 1
        return real_reduce(*args, **kw)

    def counted_all():
        counts["rounds"] += 1
        local_accum.append(step.accum.clone())
        real_all()

    dist.all_reduce = counted_reduce
    step.sync.all = counted_all

    nb = 5
    due = accum_updates(nb, 3)
    step.begin_epoch(nb)
    window_ok = None
    pending_ok = True
    for i in range(nb):
        batch = [torch.from_numpy(x).to(dev) for x in synthetic_batch(a.batch, 18, 11, 6, 1000 * rank + i)]
        counts["on"] = True
        step(*batch)
        counts["on"] = False
        pending_ok = pending_ok and step.pending == (0 if due[i] else (i - 1) % 3 + 1)
        if i == 3:  # the end of the first window of three
            torch.cuda.synchronize()
            mine = local_accum[-1]
            parts = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            want = parts[0].clone()
            for t in parts[1:]:
                want += t
            window_ok = bool(torch.equal(step.accum.view(torch.int32), want.view(torch.int32)))
    dist.all_reduce = real_reduce
    torch.cuda.synchronize()
    p = model.flat_parameters()
    gathered = [torch.empty_like(p) for _ in range(world)]
    dist.all_gather(gathered, p.contiguous())
    same = all(torch.equal(gathered[0], g) for g in gathered[1:])
    moved = float((p - p0).abs().max())
    res = {"world": world, "backend": a.backend, "replicas_identical": bool(same), "max_param_change": moved,
           "all_reduce_rounds": counts["rounds"], "all_reduce_calls": counts["calls"], "updates_due": due,
           "window_sum_bitwise": window_ok, "pending_ok": bool(pending_ok), "steps_taken": step.steps_taken()}
    if rank == 0:
        print(json.dumps(res), flush=True)
    dist.destroy_process_group()
    ok = same and moved > 0.0 and counts["rounds"] == 3 and window_ok and pending_ok and res["steps_taken"] == 3
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
