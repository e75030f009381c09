"""The training loop of the reference's train.py on the device: a command line over daimc_amd.train.Trainer.

    python tools/train_loop.py --batch 50 --epochs 4 --rounds 100 --folder runs/a [--resume] [--sprites dsprites.npz] [--report | --report-mi]

Per epoch: the gamma schedule, `rounds` training rounds (one engine call each, no read-back), the evaluation block on `--test-size`
random transitions, one line in the reference's format, and a checkpoint (model.save_all: weights, stats, optimiser state) every second
epoch, as train.py:128-129.  --sprites takes the dSprites archive (an .npz with `imgs`, or an .npy of [N,64,64] uint8); without it the
games run on the synthetic sprite bank, because the archive does not ship.  There are no plots.  With --report the epoch evaluation is
Trainer.report: the same numbers reduced on the device and downloaded once, and `stats` gains `mse_r` (the reward-transition test) and
`spearman` (latent against true factor, [10, 6] per epoch); the printed line is the same.  --report-mi is --report with `mutual_info` as
well: the k-nearest-neighbour mutual information of every latent with every true factor ([10, 6] per epoch), in the same download."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parser():
    from daimc_amd.train import DEFAULTS as D
    ap = argparse.ArgumentParser(description='Training loop on the device (train.py of the reference).')
    ap.add_argument('-r', '--resume', action='store_true', help='load the checkpoint in --folder and continue from its last epoch')
    ap.add_argument('-b', '--batch', type=int, default=D['batch'], help='games per round (train.py: 50)')
    ap.add_argument('--epochs', type=int, default=D['epochs'])
    ap.add_argument('--rounds', type=int, default=D['rounds'], help='training rounds per epoch (train.py: ROUNDS)')
    ap.add_argument('--test-size', type=int, default=D['test_size'], help='transitions of the evaluation batch (train.py: TEST_SIZE)')
    ap.add_argument('--folder', default='train_run', help='the checkpoint lives in FOLDER/checkpoints')
    ap.add_argument('--sprites', default=None, metavar='PATH', help='dSprites images; default: the synthetic sprite bank')
    ap.add_argument('--report', action='store_true', help='evaluate through Trainer.report: one download per epoch, stats gain mse_r and spearman')
    ap.add_argument('--report-mi', action='store_true', help='--report, and stats gain mutual_info: the KSG mutual information of every latent with every true factor')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    return ap


def sprites(path):
    if path is None:
        return None
    import numpy as np
    z = np.load(path, allow_pickle=False)
    return z['imgs'] if hasattr(z, 'files') else z


def epoch_line(epoch, st, dur):
    """train.py:189-193"""
    return (f"{epoch}, F: {st['F']:.2f}, MSEo: {st['mse_o']:.3f}, KLs: {st['kl_div_s']:.2f}, omega: {st['omega']:.2f}+-{st['omega_std']:.2f}, "
            f"KLpi: {st['kl_div_pi']:.2f}, TC: {st['TC']:.2f}, dur. {dur:.2f}s")


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    import daimc_amd
    from daimc_amd.train import DEFAULTS as D, EVAL_KEYS, REPORT_KEYS, Trainer, make_batch_random
    chp = os.path.join(args.folder, 'checkpoints')
    os.makedirs(chp, exist_ok=True)
    model = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device=args.device, seed=args.seed)      # train.py:33-37, 61
    imgs = sprites(args.sprites)
    games = daimc_amd.Game(args.batch, model=model, imgs=imgs, seed=args.seed)
    game_test = daimc_amd.Game(args.test_size, model=model, imgs=imgs, seed=args.seed + 1)
    report = args.report or args.report_mi
    keys = (REPORT_KEYS + (('mutual_info',) if args.report_mi else ())) if report else EVAL_KEYS
    stats, optimizers = ({k: [] for k in keys}, None)
    if args.resume:                                                                                      # train.py:76-83
        stats, optimizers = model.load_all(chp)
        for k in keys:
            stats.setdefault(k, [])
    gen = torch.Generator(device=model.device).manual_seed(args.seed)
    tr = Trainer(model, games, optimizers, lr_top=D['lr_top'], lr_mid=D['lr_mid'], lr_down=D['lr_down'], generator=gen)
    start = time.time()
    for epoch in range(len(stats['F']) + 1, args.epochs + 1):
        tr.begin_epoch(epoch)
        tr.epoch(args.rounds)
        st = tr.report(game_test, mutual_info=args.report_mi) if report else tr.evaluate(*make_batch_random(game_test, tr.repeats, gen))
        for k in keys:
            stats[k].append(st[k])
        if epoch % 2 == 0:                                                                               # train.py:128-129
            model.save_all(chp, stats, sys.argv[0], optimizers=tr.optimizers)
        print(epoch_line(epoch, st, time.time() - start), flush=True)
        start = time.time()


if __name__ == '__main__':
    main()
