"""`python -m text2human_amd.sample_from_parsing -opt configs/sample_from_parsing.yml`

The reference's sample_from_parsing.py entry point on this package: same YAML, same
dataset tree, same output files ({results_root}/{img_name}).  `--batch-size` overrides the
reference's hard-coded 4 (larger batches are what the MI355X path is built for).  By default the
images drawn for a batch depend on the batch composition through the shared RNG stream, exactly
as in the reference; with `--per-image-seeds` (YAML: `per_image_seeds: true`) every image is
drawn from a stream of its own, seeded from (`manual_seed`, its `img_name`), and its sampled
tokens no longer depend on the batch size, the batch it rides in, the shard or the rank
(DESIGN.md 4.6h).

Several GPUs of one node: launch one process per GPU,

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
           -m text2human_amd.sample_from_parsing -opt configs/sample_from_parsing.yml --batch-size 32

Rank r takes the contiguous slice `shard.shard_range(len(dataset), r, world)` of the dataset (images are
independent: no data-path collective), seeds ITS shard with `manual_seed` -- so the oracle of rank r's images is
the reference run on that same slice with that seed --, runs `model.inference` over its own loader and writes its
own PNGs into the shared results directory, which rank 0 creates (an existing one is an error on every rank, like
the reference's `make_exp_dirs`).  The `.pth` files are read once, on rank 0, and reach the other ranks over RCCL
(`shard.broadcast_state_dicts`); the only other collectives are two barriers."""
import argparse
import logging
import os
import os.path as osp
import random

import torch

from . import options, shard, weights
from .data import DeepFashionAttrPoseDataset, DeepFashionAttrSegmDataset
from .models import create_model


def dist_env():
    """(rank, world, local_rank) of a torch.distributed.run launch; (0, 1, 0) for a plain `python -m`."""
    return int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1)), int(os.environ.get('LOCAL_RANK', 0))


def init_dist(rank, world, local_rank):
    """One process per GPU: device = LOCAL_RANK, backend nccl (= RCCL over xGMI).  Without a GPU (the world-size-2
    tests of the host logic) gloo.  -> the torch.distributed module, or None for a single process."""
    if world == 1 and os.environ.get('T2H_FORCE_DIST') != '1':  # (T2H_FORCE_DIST=1: a one-rank group, test hook)
        return None
    import torch.distributed as dist
    if world == 1:
        os.environ.setdefault('RANK', '0')
        os.environ.setdefault('WORLD_SIZE', '1')
        os.environ.setdefault('MASTER_PORT', '29533')
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
    else:
        dist.init_process_group('gloo')
    return dist


def _setup(opt_path, log_name, rank=0, world=1, dist=None):
    opt = options.parse(opt_path, is_train=False)
    # the results directory: made by rank 0 (FileExistsError if it exists, utils/util.py:22); every rank learns the
    # outcome before going on, so that no rank waits at a barrier for one that has raised
    err = [None]
    if rank == 0:
        try:
            options.make_exp_dirs(opt)
        except FileExistsError as e:
            err[0] = str(e)
    if dist is not None:
        dist.broadcast_object_list(err, src=0)
    if err[0] is not None:
        raise FileExistsError(err[0])
    logger = logging.getLogger('base')
    logger.setLevel(logging.INFO)
    fmt = logging.Formatter('%(asctime)s %(levelname)s: %(message)s' if world == 1 else
                            f'%(asctime)s %(levelname)s [rank {rank}/{world}]: %(message)s')
    handlers = [logging.StreamHandler()]
    if rank == 0:  # one log file, rank 0's (the reference's name)
        handlers.append(logging.FileHandler(osp.join(opt['path']['log'], f"{log_name}_{opt['name']}.log")))
    for handler in handlers:
        handler.setFormatter(fmt)
        logger.addHandler(handler)
    if rank == 0:
        logger.info(options.dict2str(opt))
    opt = options.dict_to_nonedict(opt)
    seed = opt['manual_seed']
    if seed is None:
        seed = [random.randint(1, 10000)]
        if dist is not None:
            dist.broadcast_object_list(seed, src=0)
        seed = seed[0]
    logger.info(f'Random seed: {seed}')
    opt['manual_seed'] = seed  # (the run's seed, drawn or given: per_image_seeds derives every image's seed from it)
    options.set_random_seed(seed)  # every rank seeds ITS shard with the run's seed
    return opt, logger


def cli_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('-opt', type=str, required=True, help='Path to option YAML file.')
    ap.add_argument('--batch-size', type=int, default=4)
    ap.add_argument('--order', choices=options.SAMPLE_ORDERS, default=None,
                    help='index sampler: the reference\'s random-order loop or confidence-ordered parallel decoding '
                         '(overrides sample_order of the YAML)')
    ap.add_argument('--rounds', type=int, default=None, help='rounds of --order confidence (overrides confidence_rounds)')
    ap.add_argument('--top-k', type=int, default=None,
                    help='index sampler: draw every token among its k most likely classes (overrides sample_top_k)')
    ap.add_argument('--top-p', type=float, default=None,
                    help='index sampler: draw every token from the most likely classes that hold this share of the '
                         'probability (overrides sample_top_p)')
    ap.add_argument('--best-of', type=int, default=None,
                    help='index sampler: draw N candidates per batch and keep, per image, the one with the highest mean '
                         'log-probability per drawn token (overrides sample_best_of; 1: off)')
    ap.add_argument('--refine-temp', type=float, default=None,
                    help='refinement: draw the bottom (detail) indices from the index-prediction softmax at this '
                         'temperature instead of taking its mode (overrides refine_temp)')
    ap.add_argument('--refine-top-k', type=int, default=None,
                    help='refinement: draw every detail code among its k most likely classes (overrides refine_top_k)')
    ap.add_argument('--refine-top-p', type=float, default=None,
                    help='refinement: draw every detail code from the most likely classes that hold this share of the '
                         'probability (overrides refine_top_p)')
    ap.add_argument('--per-image-seeds', action='store_true', default=None,
                    help='index sampler: draw every image from a stream of its own, seeded from manual_seed and the '
                         'image\'s name -- an image no longer depends on its batch (sets per_image_seeds)')
    ap.add_argument('--revise-passes', type=int, default=None,
                    help='index sampler: self-correction passes on the sampled token map -- re-mask the tokens the '
                         'model\'s own pseudo-likelihood likes least, redraw them, keep the result where that '
                         'likelihood rose (overrides revise_passes; 0: off)')
    ap.add_argument('--revise-fraction', type=float, default=None,
                    help='self-correction: share of an image\'s tokens a pass redraws, in (0, 1] (overrides '
                         'revise_fraction; default 0.25)')
    ap.add_argument('--revise-folds', type=int, choices=options.REVISE_FOLDS, default=None,
                    help='self-correction: folds of the critic\'s lattice = its evaluations per scoring (overrides '
                         'revise_folds; default 4)')
    for name in options.RECOLOR_NAMES:
        ap.add_argument(f'--recolor-{name}', type=_rgb, default=None, metavar='R,G,B',
                        help=f'recolour the {name} garment of every image written towards this colour, three numbers in '
                             f'[0, 1]: an image-space operator on the decoded image, the sampled tokens are what they '
                             f'were (sets recolor_{name})')
    ap.add_argument('--recolor-feather', type=int, default=None,
                    help='recolouring: pixels over which the change fades outside a garment, 0 .. 8 (overrides '
                         'recolor_feather; default 2)')
    ap.add_argument('--recolor-luma', type=float, default=None,
                    help='recolouring: share of the luma difference to the target colour that is applied, in [0, 1] '
                         '(overrides recolor_luma; default 1)')
    return ap


def _rgb(text):
    """'R,G,B' -> [r, g, b] (floats; their range is checked by options.recolor_settings)"""
    try:
        vals = [float(x) for x in text.split(',')]
    except ValueError:
        vals = []
    if len(vals) != 3:
        raise argparse.ArgumentTypeError(f'expected three numbers R,G,B, got {text!r}')
    return vals


def apply_cli(opt, args):
    """The command line's overrides of the YAML's sampling keys, validated (a bad value ends the run here, before the
    checkpoints are read).  Returns opt."""
    for key, v in (('sample_order', args.order), ('confidence_rounds', args.rounds), ('sample_top_k', args.top_k),
                   ('sample_top_p', args.top_p), ('sample_best_of', args.best_of), ('refine_temp', args.refine_temp),
                   ('refine_top_k', args.refine_top_k), ('refine_top_p', args.refine_top_p),
                   ('per_image_seeds', getattr(args, 'per_image_seeds', None)),
                   ('revise_passes', getattr(args, 'revise_passes', None)),
                   ('revise_fraction', getattr(args, 'revise_fraction', None)),
                   ('revise_folds', getattr(args, 'revise_folds', None)),
                   *((f'recolor_{n}', getattr(args, f'recolor_{n}', None))
                     for n in options.RECOLOR_NAMES + ('feather', 'luma'))):
        if v is not None:
            opt[key] = v
    options.sampling_order(opt)
    options.sampling_truncation(opt)
    options.sampling_best_of(opt)
    options.refine_sampling(opt)
    options.per_image_seeding(opt)
    options.revise_settings(opt)
    options.recolor_settings(opt)
    return opt


def run(pose=False, argv=None):
    args = cli_parser().parse_args(argv)
    rank, world, local_rank = dist_env()
    dist = init_dist(rank, world, local_rank)
    try:
        opt, logger = _setup(args.opt, 'test', rank, world, dist)
        apply_cli(opt, args)
        if pose:
            dataset = DeepFashionAttrPoseDataset(pose_dir=opt['pose_dir'], texture_ann_dir=opt['texture_ann_file'],
                                                 shape_ann_path=opt['shape_ann_path'])
        else:
            dataset = DeepFashionAttrSegmDataset(img_dir=opt['test_img_dir'], segm_dir=opt['segm_dir'],
                                                 pose_dir=opt['pose_dir'], ann_dir=opt['test_ann_file'])
        n_total = len(dataset)
        if dist is not None:
            lo, hi = shard.shard_range(n_total, rank, world)
            dataset = torch.utils.data.Subset(dataset, range(lo, hi))
            logger.info(f'Number of test set: {n_total}; this rank: items [{lo}, {hi}).')
        else:
            logger.info(f'Number of test set: {n_total}.')
        loader = torch.utils.data.DataLoader(dataset=dataset, batch_size=args.batch_size, shuffle=False)
        if dist is not None:
            dev = torch.device('cuda', local_rank) if torch.cuda.is_available() else torch.device('cpu')
            # the `.pth` files are read by rank 0 alone; its outcome reaches every rank BEFORE the broadcast, so that a
            # missing / corrupt checkpoint ends all ranks with the error instead of leaving the others blocked in a
            # collective until the RCCL timeout
            sds0, err = None, [None]
            if rank == 0:
                try:
                    sds0 = load_state_dicts(opt)
                except Exception as e:  # noqa: BLE001 -- whatever the loader raised, every rank must learn it
                    err[0] = f'{type(e).__name__}: {e}'
            dist.broadcast_object_list(err, src=0)
            if err[0] is not None:
                raise RuntimeError(f'rank 0 could not load the checkpoints: {err[0]}')
            # (the helper's `world` argument is its "is distributed" switch)
            sds = shard.broadcast_state_dicts(sds0, 2, dev)
            model = create_model(opt, state_dicts=sds)
        else:
            model = create_model(opt)
        model.inference(loader, opt['path']['results_root'])
        if dist is not None:
            dist.barrier()  # every rank's files are on disk when any rank returns
    finally:
        if dist is not None and dist.is_initialized():
            dist.destroy_process_group()


def load_state_dicts(opt):
    """The `.pth` files named by the YAML, read once (rank 0 of a multi-GPU launch)."""
    return weights.load_checkpoints(opt)


if __name__ == '__main__':
    run(pose=False)
