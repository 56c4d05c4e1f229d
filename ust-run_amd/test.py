#!/usr/bin/env python3
"""test.py -- MI355X build of the reference's evaluation driver (test.py:19-250).

Same command line (flag names and defaults of test.py:19-32; `--dataset` also accepts BUSI, which the reference
trains but does not list here); additive flags: --synthetic, --data_root, --test_batches, --backend_dtype, --seed, --surface_metrics,
--save_dir, --save_img_mode, --post_process, --volume_metrics, --case_pattern, --voxelspacing, --volume_post_process.  Loads
`../model/<dataset>/<save_name>/unet_avg_dice_best_model.pth` (a plain state_dict with the reference's keys, test.py:241)
and prints the per-domain and mean Dice of ustrun.evaluate.validate; `--surface_metrics 1` adds the reference's
dc / jc / hd / asd lines (test.py:117-136,160-176), computed on the device instead of with medpy.  `--save_img` writes the
reference's one picture per test image (test.py:110-113) under ./img/save (or --save_dir), rendered on the device
(ustrun/render.py); `--save_img_mode contour` draws the library's other view, prediction against ground truth.
`--post_process 1` runs every part of the prediction through the reference's post_processing (dataloaders/utils.py:193-204) on the
device before it is measured or drawn.  `--volume_metrics 1 --case_pattern RE [--voxelspacing z,y,x]` (with --synthetic 0) also groups
every domain's test slices into cases by `re.match(RE, name).group(1)`, stacks each case's predictions to a volume on the device and logs
medpy's dc / jc / hd95 / asd / assd per case volume, averaged per domain (ustrun.evaluate.validate_volumes);
`--volume_post_process 1` runs each case's stacked prediction through the reference's post_processing as a VOLUME first (cavities
filled, components below a fifth of the case's foreground removed: ustrun_post_process_3d), 2 also keeps only each part's largest
component.  `--post_process` keeps meaning the per-slice rule in `validate`.  Batches come from the seeded synthetic generator, or with --synthetic 0 from the test splits under --data_root (ustrun/datasets.py).
"""
import argparse
import logging
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

parser = argparse.ArgumentParser()
parser.add_argument('--dataset', type=str, default='prostate', choices=['fundus', 'prostate', 'MNMS', 'BUSI'])
parser.add_argument("--save_name", type=str, default="debug", help="experiment_name")
parser.add_argument("--overwrite", action='store_true')
parser.add_argument("--model", type=str, default="unet", help="model_name")
parser.add_argument("--gpu", type=str, default='0')
parser.add_argument('--eval', type=bool, default=True)
parser.add_argument("--test_bs", type=int, default=1)
parser.add_argument('--domain_num', type=int, default=6)
parser.add_argument('--lb_domain', type=int, default=1)
parser.add_argument('--save_img', action='store_true')
# additive flags of this build
parser.add_argument('--synthetic', type=int, default=1)
parser.add_argument('--test_batches', type=int, default=8, help='synthetic batches per domain')
parser.add_argument('--data_root', type=str, default='../../data', help='--synthetic 0: where the dataset folders are')
parser.add_argument('--backend_dtype', default='f32', choices=['f32', 'f32x3', 'bf16', 'f16'])
parser.add_argument('--seed', type=int, default=1337)
parser.add_argument('--load_path', type=str, default='', help='state_dict file (default: the reference\'s path)')
parser.add_argument('--backbone', default='resnet101', choices=['resnet50', 'resnet101'], help='--model deeplabv2')
parser.add_argument('--surface_metrics', type=int, default=0, choices=[0, 1], help='1: also dc / jc / hd95 / asd per part')
parser.add_argument('--image_size', type=int, default=0, help='patch extent override (0: the dataset default)')
parser.add_argument('--save_dir', type=str, default='./img/save', help='--save_img: where the pictures go (test.py:113)')
parser.add_argument('--save_img_mode', default='mask', choices=['mask', 'contour'],
                    help='--save_img: draw_mask_and_save (the reference\'s) or draw_contour_and_save')
parser.add_argument('--post_process', type=int, default=0, choices=[0, 1],
                    help='1: fill holes and drop components below a fifth of the foreground before measuring')
parser.add_argument('--volume_metrics', type=int, default=0, choices=[0, 1],
                    help='1: also dc / jc / hd95 / asd / assd per case volume (needs --synthetic 0 and --case_pattern)')
parser.add_argument('--case_pattern', type=str, default='', help='--volume_metrics: regular expression whose group 1 names the case of a slice')
parser.add_argument('--voxelspacing', type=str, default='', help='--volume_metrics: z,y,x spacing of a voxel (default: voxel units)')
parser.add_argument('--volume_post_process', type=int, default=0, choices=[0, 1, 2],
                    help='--volume_metrics: 1: post-process every case as a volume before measuring; 2: and keep its largest component only')

DOMAINS = {"fundus": 4, "prostate": 6, "MNMS": 4, "BUSI": 1}     # test.py:209-223


def make_loaders(args, C, H):
    if not args.synthetic:      # the reference's per-domain test splits (test.py:222-230), resident, no augmentation
        from ustrun import datasets
        return datasets.test_loaders(datasets.test_datasets(args, H, "cuda"), args.test_bs)
    from ustrun import synthetic
    return synthetic.test_loaders(args.dataset, args.domain_num, args.test_batches, args.test_bs, C, H, args.seed)


def main(args):
    from networks.unet_model import UNet
    from ustrun.evaluate import validate
    from ustrun.trainer import DATASETS
    C, H, K = DATASETS[args.dataset][:3]
    H = args.image_size or H
    args.domain_num = min(args.domain_num, DOMAINS[args.dataset])
    if args.volume_metrics and (args.synthetic or not args.case_pattern):
        raise SystemExit("--volume_metrics 1 groups the slices of a dataset's test split: it needs --synthetic 0 and --case_pattern")
    if args.volume_post_process and not args.volume_metrics:
        raise SystemExit("--volume_post_process cleans the case volumes --volume_metrics 1 measures: it needs --volume_metrics 1")
    if args.model not in ('unet', 'deeplabv2'):
        raise SystemExit("--model is 'unet' (the reference's path) or 'deeplabv2' (train.py --model deeplabv2 of this build)")
    if args.model == 'deeplabv2':
        from networks.deeplabv2 import DeepLabV2
        model = DeepLabV2(args.backbone, K, pretrained=False, dtype=args.backend_dtype).cuda()
    else:
        model = UNet(n_channels=C, n_classes=K, dtype=args.backend_dtype).cuda()
    path = args.load_path or '../model/{}/{}/{}_avg_dice_best_model.pth'.format(args.dataset, args.save_name, args.model)
    model.load_state_dict(torch.load(path, map_location="cuda"))
    out = validate(args.dataset, model, make_loaders(args, C, H), epoch=args.lb_domain, surface_metrics=bool(args.surface_metrics),
                   save_dir=args.save_dir if args.save_img else None, save_mode=args.save_img_mode,
                   post_process=bool(args.post_process))
    if args.volume_metrics:
        from ustrun import datasets
        from ustrun.evaluate import validate_volumes
        spacing = tuple(float(v) for v in args.voxelspacing.split(',')) if args.voxelspacing else None
        validate_volumes(args.dataset, model, datasets.test_datasets(args, H, "cuda"), args.case_pattern, spacing,
                         post_process=args.volume_post_process >= 1, largest=args.volume_post_process == 2)
    return out


if __name__ == "__main__":
    args = parser.parse_args()
    os.environ.setdefault("HIP_VISIBLE_DEVICES", args.gpu)
    logging.basicConfig(level=logging.INFO, format='[%(asctime)s.%(msecs)03d] %(message)s', datefmt='%H:%M:%S',
                        handlers=[logging.StreamHandler(sys.stdout)])
    logging.info(str(args))
    main(args)
