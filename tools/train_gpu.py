"""train_mpi.py on the MI355X with synthetic batches (no dataset download on the GPU box).

    python tools/train_gpu.py --workers 8 --epoch 2 --batches 50                 # 8 virtual workers, 1 GPU
    python tools/train_gpu.py --compress --budget 0.5                           # ChocoSGD
    python tools/train_gpu.py --momentum 0.9 --fused-sgd                        # SGD step fused into the round
    python tools/train_gpu.py --momentum 0.9 --fused-sgd --bf16                 # the same, bf16 models + fp32 masters
    python tools/train_gpu.py --lr 1e-3 --no-warmup --fused-adamw --wd 1e-2       # AdamW step fused into the round
    python tools/train_gpu.py --lr 1e-3 --no-warmup --fused-adamw --wd 1e-2 --bf16 # the same, bf16 models + fp32 masters
    python tools/train_gpu.py --lr 1e-4 --no-warmup --fused-lion --wd 1e-2 --bf16 --lion-bf16-momentum
                                                                                # Lion fused in, 18 bytes / parameter
    python tools/train_gpu.py --fused-qgm --qgm-mu 0.9 --nesterov --bf16          # quasi-global momentum fused in
    python tools/train_gpu.py --fused-gt --momentum 0.9 --nesterov --bf16         # gradient tracking (GT-DSGD)
    torchrun --nproc-per-node N --master-addr 127.0.0.1 tools/train_gpu.py     # one worker per GPU

Flags follow train_mpi.py:205-231 (same names and defaults where they apply); --workers,
--batches, --checkpoint and --resume are the harness's own.
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("270-matcha-a-matching-based-link-scheduling-strategy-to-speed-up-distributed-optimization_amd")
H = pkg.harness


def main():
    ap = argparse.ArgumentParser(description="MI355X gossip training harness (synthetic data)")
    ap.add_argument("--name", default="Vanilla DecenSGD-synthetic")
    ap.add_argument("--description", default="MI355X gossip harness, synthetic batches")
    ap.add_argument("--model", default="mlp")
    ap.add_argument("--lr", default=0.8, type=float)
    ap.add_argument("--momentum", default=0.0, type=float)
    ap.add_argument("--epoch", "-e", default=1, type=int)
    ap.add_argument("--bs", default=64, type=int)
    ap.add_argument("--no-warmup", dest="warmup", action="store_false")
    ap.add_argument("--nesterov", action="store_true")
    ap.add_argument("--fixed", dest="matcha", action="store_false", help="FixedProcessor (D-PSGD)")
    ap.add_argument("--budget", default=1.0, type=float)
    ap.add_argument("--graphid", default=0, type=int)
    ap.add_argument("--savePath", default="./saveModel")
    ap.add_argument("--save", action="store_true")
    ap.add_argument("--compress", action="store_true")
    ap.add_argument("--compressor", default=None, choices=("topk", "sign"), help="--compress: the message -- topk "
                    "(default: the reference's top 10 %) or sign (the scaled-sign 1-bit quantizer; one process)")
    ap.add_argument("--consensus_lr", default=0.1, type=float)
    ap.add_argument("--randomSeed", default=1234, type=int)
    ap.add_argument("--workers", default=8, type=int)
    ap.add_argument("--batches", default=20, type=int, help="batches per epoch")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--batched", action="store_true", help="one vmap'd step for all virtual workers")
    ap.add_argument("--graph", action="store_true", help="with --batched: replay each iteration (step + "
                    "gossip round) as one captured HIP graph once the learning rate is constant")
    ap.add_argument("--fused-sgd", action="store_true", help="one GPU, per-worker (non-batched) training: the "
                    "workers' optimizer.step() / zero_grad() and the gossip round as ONE launch per iteration")
    ap.add_argument("--fused-adamw", action="store_true", help="as --fused-sgd with AdamW's update in the launch "
                    "(--beta1 --beta2 --eps --wd; --lr is AdamW's, e.g. 1e-3)")
    ap.add_argument("--fused-lion", action="store_true", help="as --fused-sgd with the Lion update in the launch "
                    "(--beta1 --beta2 --wd; --lr is Lion's, e.g. 1e-4)")
    ap.add_argument("--lion-bf16-momentum", action="store_true", help="--fused-lion --bf16: keep the momentum in "
                    "bfloat16 too (18 instead of 22 bytes per parameter and round)")
    ap.add_argument("--fused-qgm", action="store_true", help="as --fused-sgd with quasi-global momentum (QG-DSGDm) in "
                    "the launch: the momentum buffer follows the rows' displacement after the round (--momentum "
                    "--nesterov --qgm-mu; weight decay 5e-4 as --fused-sgd)")
    ap.add_argument("--qgm-mu", default=None, type=float, metavar="X", help="--fused-qgm: the buffer's own averaging "
                    "factor mu in [0, 1) (default: --momentum, the paper's setting)")
    ap.add_argument("--fused-gt", action="store_true", help="as --fused-sgd with gradient tracking (GT-DSGD): every "
                    "worker steps along a gossiped tracker of the mean gradient, two launches per iteration "
                    "(--momentum --nesterov; weight decay 5e-4 as --fused-sgd)")
    ap.add_argument("--beta1", default=0.9, type=float)
    ap.add_argument("--beta2", default=None, type=float, help="default 0.999 (--fused-adamw) / 0.99 (--fused-lion)")
    ap.add_argument("--eps", default=1e-8, type=float)
    ap.add_argument("--wd", default=5e-4, type=float, help="--fused-adamw / --fused-lion: the decoupled weight decay")
    ap.add_argument("--bf16", action="store_true", help="one GPU: the models are cast to bfloat16 (bfloat16 gossip "
                    "rows); with --fused-sgd / --fused-adamw the step runs in mixed precision on fp32 master weights, which the "
                    "round mixes, and the bfloat16 models are their rounded image")
    ap.add_argument("--pull", action="store_true", help="one process per GPU: gossip rounds over the pull "
                    "transport (partner rows / Choco messages read from the peers' HBM) instead of RCCL")
    ap.add_argument("--clip-grad-norm", default=None, type=float, metavar="X", help="--fused-sgd / --fused-adamw: "
                    "torch.nn.utils.clip_grad_norm_(model.parameters(), X) per worker inside the fused step (one "
                    "extra read of the gradients); an error on the paths that keep torch's optimizers")
    ap.add_argument("--no-decay-1d", action="store_true", help="--fused-sgd / --fused-adamw: weight decay 0 for "
                    "parameters with ndim <= 1 (biases, normalisation scales), as a parameter group of the fused "
                    "step; an error on the paths that keep torch's optimizers")
    ap.add_argument("--consensus-every", default=None, type=int, metavar="K", help="one GPU: measure how far apart "
                    "the workers are after every K-th iteration's round (one read of the rows, no host wait per "
                    "round) and print the consensus distance and its ratio to the norm of the mean per epoch")
    ap.add_argument("--slowmo-every", default=None, type=int, metavar="K", help="one GPU, with a --fused-* step: "
                    "SlowMo's outer step after every K-th iteration's round -- the workers' exact average, moved by a "
                    "slow momentum, becomes every worker's row (one launch)")
    ap.add_argument("--slowmo-beta", default=None, type=float, metavar="X", help="--slowmo-every: the slow momentum "
                    "factor in [0, 1) (default 0.5)")
    ap.add_argument("--slowmo-alpha", default=None, type=float, metavar="X", help="--slowmo-every: the slow learning "
                    "rate, > 0 (default 1.0)")
    ap.add_argument("--slowmo-buffers", default=None, choices=("reset", "maintain", "average"), help="--slowmo-every: "
                    "what the outer step does to the base optimizer's momentum (default reset)")
    a = ap.parse_args()
    fused = a.fused_sgd or a.fused_adamw or a.fused_lion or a.fused_qgm or a.fused_gt
    if a.qgm_mu is not None and not a.fused_qgm:
        ap.error("--qgm-mu is the quasi-global momentum step's: add --fused-qgm")
    if a.compressor is not None and not a.compress:
        ap.error("--compressor chooses ChocoSGD's message: add --compress")
    if a.consensus_every is not None and a.consensus_every < 1:
        ap.error("--consensus-every: a positive number of iterations")
    slowmo = {k: v for k, v in (("beta", a.slowmo_beta), ("alpha", a.slowmo_alpha), ("buffers", a.slowmo_buffers))
              if v is not None}
    if a.slowmo_every is None and slowmo:
        ap.error("--slowmo-beta / --slowmo-alpha / --slowmo-buffers belong to --slowmo-every K")
    if a.slowmo_every is not None and (a.slowmo_every < 1 or not fused):
        ap.error("--slowmo-every: a positive number of iterations, with one of the --fused-* steps")
    if a.no_decay_1d and not fused:
        ap.error("--no-decay-1d is honoured by the fused optimizer steps only: add --fused-sgd, --fused-adamw or "
                 "--fused-lion")
    if a.lion_bf16_momentum and not (a.fused_lion and a.bf16):
        ap.error("--lion-bf16-momentum is the mixed-precision Lion step's: add --fused-lion --bf16")
    if a.clip_grad_norm is not None and not fused:
        ap.error("--clip-grad-norm is honoured by the fused optimizer steps only: add --fused-sgd, --fused-adamw or "
                 "--fused-lion "
                 "(the other paths step torch's optimizers and do not clip)")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if a.clip_grad_norm is not None and world > 1:
        ap.error("--clip-grad-norm: one process per GPU trains with torch's optimizers (no fused step yet) and "
                 "does not clip")
    if a.no_decay_1d and world > 1:
        ap.error("--no-decay-1d: one process per GPU trains with torch's optimizers (no fused step yet)")
    if a.slowmo_every is not None and world > 1:
        ap.error("--slowmo-every: the exact average needs every worker's rows on one GPU (one process)")
    if a.consensus_every is not None and world > 1:
        ap.error("--consensus-every: the mean needs every worker's rows on one GPU (one process)")
    args = H.HarnessArgs(name=a.name, description=a.description, model=a.model, lr=a.lr, momentum=a.momentum,
                         epoch=a.epoch, bs=a.bs, warmup=a.warmup, nesterov=a.nesterov, matcha=a.matcha,
                         budget=a.budget, graphid=a.graphid, savePath=a.savePath, save=a.save,
                         compress=a.compress, consensus_lr=a.consensus_lr, randomSeed=a.randomSeed,
                         size=a.workers if world == 1 else world)
    if a.compressor is not None:
        if a.compressor == "sign" and world > 1:
            ap.error("--compressor sign: one process (the per-GPU trainer keeps the top-k message)")
        args.compressor = a.compressor
    import torch
    model_fn = H.model_factory(args)
    if a.bf16:
        if world > 1:
            ap.error("--bf16: bfloat16 worker rows are mixed on one GPU only")
        fp32_fn = model_fn

        def model_fn():
            return fp32_fn().to(torch.bfloat16)
    if world > 1:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        tr = H.RankTrainer(args, model_fn, a.batches, rank, world,
                           transport="pull" if a.pull else None)
    else:
        tr = H.VirtualTrainer(args, model_fn, a.batches, batched=a.batched or a.graph, graph=a.graph,
                              fused_sgd=a.fused_sgd, fused_adamw=a.fused_adamw,
                              adamw_hyper={"betas": (a.beta1, 0.999 if a.beta2 is None else a.beta2), "eps": a.eps,
                                           "weight_decay": a.wd},
                              fused_lion=a.fused_lion,
                              lion_hyper={"betas": (a.beta1, 0.99 if a.beta2 is None else a.beta2), "weight_decay": a.wd,
                                          "momentum_dtype": torch.bfloat16 if a.lion_bf16_momentum else torch.float32},
                              fused_qgm=a.fused_qgm, qgm_hyper={"mu": a.qgm_mu}, fused_gt=a.fused_gt,
                              clip_grad_norm=a.clip_grad_norm,
                              param_groups=[{"params": lambda name, p: p.ndim <= 1, "weight_decay": 0.0}]
                              if a.no_decay_1d else None, consensus_every=a.consensus_every,
                              slowmo_every=a.slowmo_every, slowmo_hyper=slowmo or None)
        if a.resume:
            tr.load(a.resume)
    import time
    while tr.epoch < args.epoch:
        torch.cuda.synchronize()
        t = time.time()
        stats = tr.train_epoch()
        torch.cuda.synchronize()
        if rank == 0:
            norms = "" if "grad_norm" not in stats[0] else \
                ", grad_norm: " + " ".join(f"{s['grad_norm']:.3g}" for s in stats)
            cons = ""
            if "consensus" in stats[0]:
                xi, mean_norm = (float(v) for v in tr.consensus_log[-1][-2:])
                cons = f", consensus: {xi:.4g} (relative {xi / mean_norm if mean_norm else float('nan'):.3g})"
            print(H.epoch_summary(stats, tr.epoch - 1) + f", wall: {time.time() - t:.3f} s "
                  f"({a.batches / (time.time() - t):.1f} iterations/s)" + norms + cons, flush=True)
    tr.finish()
    if a.checkpoint and world == 1:
        tr.save(a.checkpoint)


if __name__ == "__main__":
    main()
