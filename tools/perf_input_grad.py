"""Timing of scd_input_grad (the first layer's data grad) at the bench shape, and what input gradients cost a step.

    python tools/perf_input_grad.py [--batch 64] [--size 256] [--c0 64] [--cin 5] [--rounds 7] [--reps 20]
    python tools/perf_input_grad.py --step [--config baseline_siamese --step-batch 32]

Kernel part: HIP events around `reps` launches, the median over `rounds` windows, for fp32 and bf16 storage of dy,
interleaved with (a) a device copy of the same dy, which gives the copy bandwidth of this box and the time the bytes
alone cost, and (b) scd_conv_igemm on the same dy with n_out = 16 (the generic data-grad launch: packed weights, NHWC
output), in the arithmetic it would run in a model (h2 with a bound on fp32 storage, bf16 on bf16 storage).
Step part: the config's training step with x_t1 / x_t2 requiring grad against the same step without, interleaved in
one process (the method of tools/ab_step.py).
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_siamese_cd_amd import hip  # noqa: E402


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def kernels(args):
    dev = torch.device('cuda:0')
    n, s, c0, cin = args.batch, args.size, args.c0, args.cin
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(c0, cin, 3, 3, device=dev, generator=g) * 0.05
    w16 = torch.zeros(c0, 16, 3, 3, device=dev)
    w16[:, :cin] = w
    gx = torch.empty(n, cin, s, s, device=dev)
    flop = 2.0 * n * s * s * cin * 9 * c0
    for sdt, name, math in ((torch.float32, 'fp32', 'h2'), (torch.bfloat16, 'bf16', 'bf16')):
        dy = torch.randn(n, s, s, c0, device=dev, generator=g).to(sdt)
        dy2 = torch.empty_like(dy)
        nbytes = dy.numel() * dy.element_size() + gx.numel() * 4
        out16 = torch.empty(n, s, s, 16, device=dev, dtype=sdt)
        fns = {'input_grad': lambda: hip.input_grad(hip.nhwc(dy), w, [(gx, 0, cin, 0, 0, n)]),
               'copy of dy': lambda: dy2.copy_(dy)}
        prev = hip.set_conv_math(math)
        try:
            wb = hip.pack_conv3x3(w16, 1)
            db = None
            if math == 'h2':
                db = torch.zeros(1, device=dev)
                hip.absmax_bound(hip.nhwc(dy), db)
            generic = lambda: hip.conv_igemm(hip.nhwc(dy), s, s, 1, hip.TAPS_3X3, wb, 16, None, hip.nhwc(out16),
                                             src_bound=db)
            try:
                arith = hip.igemm_arith(hip.nhwc(dy), s, s, 1, hip.TAPS_3X3, wb, 16, hip.nhwc(out16), src_bound=db)
                generic()
                fns[f'conv_igemm n_out=16 ({arith})'] = generic
            except RuntimeError as e:  # no generic kernel takes this shape in this storage
                print(f'  conv_igemm n_out=16 on {name} storage: {e}')
                out16 = None
            times = {k: [] for k in fns}
            for fn in fns.values():
                window(fn, 3)
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    times[k].append(window(fn, args.reps))
        finally:
            hip.set_conv_math(prev)
        # the generic launch's result equals the new kernel's (its real channels, NHWC)
        err = float('nan') if out16 is None else \
            ((out16[..., :cin].float().permute(0, 3, 1, 2) - gx).abs().max() / gx.abs().max()).item()
        copy_ms = statistics.median(times['copy of dy'])
        bw = 2.0 * dy.numel() * dy.element_size() / copy_ms / 1e9  # TB/s: a copy reads and writes its bytes
        print(f'dy {n}x{s}x{s}x{c0} {name}, cin {cin}: {nbytes / 1e6:.0f} MB moved, {flop / 1e9:.1f} GFLOP; copy '
              f'bandwidth of this box {bw:.2f} TB/s -> the bytes alone take {nbytes / bw / 1e9:.3f} ms; generic vs '
              f'input_grad max-relative difference {err:.1e}')
        for k, ts in times.items():
            m = statistics.median(ts)
            print(f'  {k:32s} median {m:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}'
                  + (f'  ({nbytes / m / 1e9:.2f} TB/s, {flop / m / 1e9:.1f} TFLOP/s)' if k == 'input_grad' else ''),
                  flush=True)


def step(args):
    from multimodal_siamese_cd_amd import trainers
    from multimodal_siamese_cd_amd.utils import datasets, experiment_manager, networks
    dev = torch.device('cuda:0')
    cfg = experiment_manager.load_cfg(args.config)
    batch = args.step_batch or int(cfg.TRAINER.BATCH_SIZE)
    torch.manual_seed(cfg.SEED)
    net = networks.create_network(cfg).to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), lr=float(cfg.TRAINER.LR), weight_decay=0.01, fused=True)
    b = datasets.synthetic_batch(cfg, batch, dev, torch.Generator(device=dev).manual_seed(7))

    def one(need):
        x1 = b['x_t1'].detach().requires_grad_(need)
        x2 = b['x_t2'].detach().requires_grad_(need)
        opt.zero_grad(set_to_none=True)
        trainers.step_loss(cfg, net(x1, x2), b).backward()
        opt.step()

    times = {False: [], True: []}
    for need in times:
        for _ in range(3):
            one(need)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for need in times:
            one(need)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                one(need)
            torch.cuda.synchronize()
            times[need].append(1000.0 * (time.perf_counter() - t0) / args.steps)
    m0, m1 = statistics.median(times[False]), statistics.median(times[True])
    print(f'{args.config} bs={batch}: step without input gradients median {m0:.3f} ms (min {min(times[False]):.3f}), '
          f'with x_t1 and x_t2 requiring grad {m1:.3f} ms (min {min(times[True]):.3f}): +{m1 - m0:.3f} ms '
          f'({100 * (m1 - m0) / m0:.2f}%)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--c0', type=int, default=64)
    ap.add_argument('--cin', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--config', default='baseline_siamese')
    ap.add_argument('--step-batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=8)
    args = ap.parse_args()
    hip.load_library()
    hip.ensure_device(torch.empty(1, device='cuda:0'))
    if args.step:
        step(args)
    else:
        kernels(args)


if __name__ == '__main__':
    main()
