"""The bench's 3-stream training step alone (B=256, V=18, S=6, eager; precision from F3_STEP_PREC,
default bf16x3, the headline mode), for kernel traces:
    rocprofv3 --kernel-trace -d gpurun_out/step -o run -- python tools/step_only.py [steps] [autograd]
    python tools/timeline.py gpurun_out/step/run_results.db --list
With `autograd` the step is the reference loop body through the custom ops instead of TrainStep
(opt.zero_grad(); CrossEntropyLoss()(model(x, s), y).backward(); f3.RMSprop.step(), model/main.py:112-127).
With `guard` it times TrainStep(skip_nonfinite=True) against the default step in one process, eager and
captured: windows of [steps] steps, the two alternating, the median window of each (ms/step).
With `ema` it does the same for TrainStep(ema_decay=0.999); with `ema-on` the plain run below keeps the
average (for a kernel trace of ema_update_kernel)."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def option_cost(steps, what, kw, rounds=7):
    import fall_multimodal_amd as f3
    from oracle.prng import synthetic_batch
    dev = torch.device("cuda")
    B, V, S, C = 256, 18, 6, 11
    sk, se, lb = (torch.from_numpy(x).to(dev) for x in synthetic_batch(B, V, C, S, 100))
    for captured in (False, True):
        runs = {}
        for guard in (False, True):
            model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, C, S, device=dev,
                                              precision=os.environ.get("F3_STEP_PREC", "bf16x3"))
            step = f3.TrainStep(model, B, lr=1e-3, **(kw if guard else {}))
            if captured:
                step.capture(sk, se, step.prepare(sk, se, lb))
            for _ in range(5):
                step(sk, se, lb)
            runs[guard] = (step, [])
        torch.cuda.synchronize()
        for _ in range(rounds):
            for guard in (False, True):
                step, times = runs[guard]
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(sk, se, lb)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / steps * 1e3)
        on_step = runs[True][0]
        assert on_step.skipped_steps() == 0 and on_step.steps_taken() == 5 + rounds * steps
        assert on_step.ema is None or int(on_step.n_averaged.item()) == 5 + rounds * steps
        off, on = (runs[g][1] for g in (False, True))
        print(f"{'captured' if captured else 'eager'}: {what} off {statistics.median(off):.3f} ms/step "
              f"(min {min(off):.3f} max {max(off):.3f}), {what} on {statistics.median(on):.3f} ms/step "
              f"(min {min(on):.3f} max {max(on):.3f}); {rounds} windows of {steps} steps each, alternating")


def main():
    if len(sys.argv) > 2 and sys.argv[2] == "guard":
        return option_cost(int(sys.argv[1]), "guard", {"skip_nonfinite": True})
    if len(sys.argv) > 2 and sys.argv[2] == "ema":
        return option_cost(int(sys.argv[1]), "ema", {"ema_decay": 0.999})
    import fall_multimodal_amd as f3
    from oracle.prng import synthetic_batch
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    dev = torch.device("cuda")
    B, V, S, C = 256, 18, 6, 11
    model = f3.TwoStreamSTGCAN_BiLSTM(3, {"layout": "coco_mmpose", "strategy": "spatial"}, C, S, device=dev,
                                      precision=os.environ.get("F3_STEP_PREC", "bf16x3"))
    sk, se, lb = (torch.from_numpy(x).to(dev) for x in synthetic_batch(B, V, C, S, 100))
    if len(sys.argv) > 2 and sys.argv[2] == "autograd":
        opt = f3.RMSprop(model.parameters(), lr=1e-3)
        loss_fn = torch.nn.CrossEntropyLoss()

        def step(sk, se, lb):
            opt.zero_grad()
            loss_fn(model(sk, se), lb).backward()
            opt.step()
    else:
        step = f3.TrainStep(model, B, lr=1e-3, ema_decay=0.999 if sys.argv[2:3] == ["ema-on"] else None)
    for _ in range(3):
        step(sk, se, lb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(sk, se, lb)
    t1 = time.perf_counter()  # host submission done (no per-step sync in the loop)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"{(t2 - t0) / steps * 1e3:.3f} ms/step (host submit {(t1 - t0) / steps * 1e3:.3f} ms/step)")


if __name__ == "__main__":
    main()
