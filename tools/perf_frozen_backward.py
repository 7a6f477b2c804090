"""What frozen parameters cost a backward: the engine option skip_frozen_grads on against off, at the bench shape.

    python tools/perf_frozen_backward.py [--config baseline_siamese --batch 32] [--precision bf16]
                                         [--workload saliency|finetune|both] [--rounds 7] [--steps 8]
    python tools/perf_frozen_backward.py --kernel [--kbatch 64 --size 256 --channels 64]
    python tools/perf_frozen_backward.py --tree PATH ...     # the same measurement on another checkout of the package

Workloads, each a host clock around `steps` iterations that end in a device synchronise, the arms interleaved in one
process, median and min-max over `rounds` windows (the method of tools/ab_step.py and tools/perf_input_grad.py):
  saliency   net.eval(), every parameter requires_grad False, x_t1 / x_t2 requiring grad: forward + autograd.grad.
  finetune   inc. / encoder. parameters frozen and their BatchNorms in eval mode, the rest training: a full step with
             fused AdamW over net.parameters().
The last line of a run is one JSON object with every median, for a script that alternates two checkouts (`--tree`:
that checkout's package is imported instead of this one's, built there beforehand; a checkout without the option has
one arm, reported as 'off': it computes every gradient and lets autograd discard it, which is what off means).

--kernel: scd_bn_relu_through (plain form) at a [kbatch, size, size, channels] map in fp32 and bf16 storage, HIP events
around `reps` launches, against (a) the reducing frozen form of scd_bn_relu_backward_desc on the same tensors and (b) a
device copy, which gives this box's copy bandwidth and so the time the pass' bytes alone take (one read of y and of the
gradient, one write of dy).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch


def _tree(argv):
    for i, a in enumerate(argv):
        if a == '--tree' and i + 1 < len(argv):
            return os.path.abspath(argv[i + 1])
        if a.startswith('--tree='):
            return os.path.abspath(a.split('=', 1)[1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


sys.path.insert(0, _tree(sys.argv))

from multimodal_siamese_cd_amd import engine, hip  # noqa: E402

HAS_OPTION = 'skip_frozen_grads' in engine.set_options()


def _arms():
    return (True, False) if HAS_OPTION else (False,)


def _set(on):
    if HAS_OPTION:
        engine.set_options(skip_frozen_grads=on)


def _stat(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def _interleaved(one, args):
    """{arm: [ms per iteration, per round]}: warm-up of every arm, then the arms alternating round by round."""
    times = {on: [] for on in _arms()}
    for on in times:
        _set(on)
        for _ in range(3):
            one()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for on in times:
            _set(on)
            one()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                one()
            torch.cuda.synchronize()
            times[on].append(1000.0 * (time.perf_counter() - t0) / args.steps)
    _set(True)
    return times


def _model(args, dev):
    from multimodal_siamese_cd_amd.utils import datasets, experiment_manager, networks
    cfg = experiment_manager.load_cfg(args.config)
    if args.precision:
        cfg.MODEL.PRECISION = args.precision
    batch = args.batch or int(cfg.TRAINER.BATCH_SIZE)
    torch.manual_seed(cfg.SEED)
    net = networks.create_network(cfg).to(dev)
    b = datasets.synthetic_batch(cfg, batch, dev, torch.Generator(device=dev).manual_seed(7))
    return cfg, net, b, batch


def saliency(args, dev):
    from multimodal_siamese_cd_amd.utils import loss_functions
    cfg, net, b, batch = _model(args, dev)
    net.eval()
    for p in net.parameters():
        p.requires_grad_(False)
    crit = loss_functions.get_criterion('PowerJaccardLoss')

    def one():
        x1 = b['x_t1'].detach().requires_grad_()
        x2 = b['x_t2'].detach().requires_grad_()
        out = net(x1, x2)
        out = out if isinstance(out, torch.Tensor) else out[0]
        torch.autograd.grad(crit(out, b['y_change']), [x1, x2])

    return _report('saliency (eval, all frozen, forward + input gradients)', args, batch, net, _interleaved(one, args))


def finetune(args, dev):
    from multimodal_siamese_cd_amd import trainers
    cfg, net, b, batch = _model(args, dev)
    prefixes = ('inc.', 'encoder.')
    for k, p in net.module.named_parameters():
        if k.startswith(prefixes):
            p.requires_grad_(False)
    opt = torch.optim.AdamW(net.parameters(), lr=float(cfg.TRAINER.LR), weight_decay=0.01, fused=True)

    def one():
        net.train()
        for k, m in net.module.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d) and k.startswith(prefixes):
                m.eval()
        opt.zero_grad(set_to_none=True)
        trainers.step_loss(cfg, net(b['x_t1'], b['x_t2']), b).backward()
        opt.step()

    return _report('finetune (frozen encoder + its BatchNorm, full AdamW step)', args, batch, net,
                   _interleaved(one, args))


def _report(what, args, batch, net, times):
    res = {('on' if on else 'off'): _stat(ts) for on, ts in times.items()}
    line = f'{args.config} bs={batch} {net.module.conv_math}: {what}: ' + '; '.join(
        f'skip_frozen_grads {k} median {v["median"]:.3f} ms (min {v["min"]:.3f}, max {v["max"]:.3f})'
        for k, v in res.items())
    if len(res) == 2:
        d = res['off']['median'] - res['on']['median']
        line += f': on is {d:.3f} ms ({100 * d / res["off"]["median"]:.2f}%) faster'
    print(line, flush=True)
    return res


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def kernel(args, dev):
    n, s, c = args.kbatch, args.size, args.channels
    g = torch.Generator(device=dev).manual_seed(1)
    gamma, beta = torch.rand(c, device=dev, generator=g) + 0.5, torch.randn(c, device=dev, generator=g)
    rm, rv = torch.randn(c, device=dev, generator=g), torch.rand(c, device=dev, generator=g) + 0.5
    nseg = 2
    co = [torch.empty(nseg * c, device=dev) for _ in range(4)]
    hip.bn_frozen_coeffs(c, nseg, gamma, beta, rm, rv, 1e-5, *co)
    res = {}
    for sdt, name in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16')):
        y = torch.randn(n, s, s, c, device=dev, generator=g).to(sdt)
        da = torch.randn(n, s, s, c, device=dev, generator=g).to(sdt)
        dy, dy2 = torch.empty_like(y), torch.empty_like(y)
        sums = [torch.empty(c, device=dev) for _ in range(3)]
        ws = torch.empty(hip.bn_workspace_bytes(n, s, s, c, nseg), dtype=torch.uint8, device=dev)
        bound = torch.zeros(1, device=dev)
        fns = {'bn_relu_through': lambda: hip.bn_relu_through(hip.BN_BWD_PLAIN, hip.nhwc(y), nseg, co[0], co[1], gamma,
                                                              co[2], co[3], hip.nhwc(dy), bound, da=hip.nhwc(da)),
               'frozen reducing form': lambda: hip.bn_relu_backward(hip.nhwc(y), hip.nhwc(da), nseg, co[0], co[1],
                                                                    gamma, co[2], co[3], *sums, hip.nhwc(dy2), ws,
                                                                    bound, frozen=True),
               'copy of y': lambda: dy2.copy_(y)}
        times = {k: [] for k in fns}
        for fn in fns.values():
            window(fn, 3)
        fns['frozen reducing form']()  # (the warm-up's last launch was the copy into dy2)
        same = torch.equal(dy, dy2)
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(window(fn, args.reps))
        nbytes = 3 * y.numel() * y.element_size()
        copy_ms = statistics.median(times['copy of y'])
        bw = 2.0 * y.numel() * y.element_size() / copy_ms / 1e9  # TB/s: a copy reads and writes its bytes
        print(f'y {n}x{s}x{s}x{c} {name}: the pass moves {nbytes / 1e6:.0f} MB; copy bandwidth of this box {bw:.2f} TB/s '
              f'-> the bytes alone take {nbytes / bw / 1e9:.3f} ms; dy bit-equal to the reducing form: {same}')
        for k, ts in times.items():
            m = statistics.median(ts)
            print(f'  {k:24s} median {m:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}'
                  + (f'  ({nbytes / m / 1e9:.2f} TB/s)' if k == 'bn_relu_through' else ''), flush=True)
        res[name] = {k: _stat(ts) for k, ts in times.items()}
        res[name]['copy_TBps'] = bw
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=None, help='import the package from this checkout instead')
    ap.add_argument('--config', default='baseline_siamese')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--precision', default=None, choices=['fp32', 'bf16'])
    ap.add_argument('--workload', default='both', choices=['saliency', 'finetune', 'both'])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--kbatch', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    hip.load_library()
    dev = torch.device('cuda:0')
    hip.ensure_device(torch.empty(1, device=dev))
    out = {'tree': _tree(sys.argv), 'has_option': HAS_OPTION, 'precision': args.precision or 'config'}
    if args.kernel:
        out['kernel'] = kernel(args, dev)
    else:
        if args.workload in ('saliency', 'both'):
            out['saliency'] = saliency(args, dev)
        if args.workload in ('finetune', 'both'):
            out['finetune'] = finetune(args, dev)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
