"""`validate(..., save_dir=...)` and `test.py --save_img` (the reference's test.py:110-113): the pictures are written under the
reference's names, hold what ustrun.render draws, and the run returns what a run without them returns."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DATASET, C, K, H = "prostate", 1, 2, 48


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


@pytest.fixture(scope="module")
def setup():
    from networks.unet_model import UNet
    from ustrun import synthetic
    torch.manual_seed(4)
    model = UNet(C, K, base_channels=8).cuda()
    loaders = synthetic.test_loaders(DATASET, 2, 3, 2, C, H, seed=5)       # two domains, three batches of two
    return model, loaders


def _expected(model, loaders, mode, dataset=DATASET):
    """names and pictures, one loader batch at a time"""
    from ustrun import render
    from ustrun.evaluate import PARTS, predict, sample_dice
    from ustrun.trainer import decode_labels
    names, pics, num, parts = [], [], 0, len(PARTS[dataset])
    model.eval()
    with torch.no_grad():
        for dom, loader in enumerate(loaders):
            for image, label in loader:
                image, label = image.cuda(), label.cuda()
                pred, mask = predict(dataset, model(image)), decode_labels(dataset, label)
                d = sample_dice(dataset, pred, mask)
                dice = [float(sum(d[:, p]) / len(d)) for p in range(d.shape[1])]
                avg = sum(dice) / len(dice)
                rgb = (render.render_mask(image, pred, parts=parts) if mode == "mask" else
                       render.render_contour(image, pred, mask, parts=parts))
                for j in range(len(image)):
                    num += 1
                    names.append("{}_{}_{}.png".format(dom + 1, num, round(avg, 4)))
                    pics.append(rgb[j].cpu().numpy())
    model.train()
    return names, pics


@pytest.mark.parametrize("mode", ["mask", "contour"])
def test_validate_writes_the_reference_file_names_and_the_rendered_pixels(setup, tmp_path, mode):
    from ustrun.evaluate import validate
    model, loaders = setup
    plain_lines, saved_lines = [], []
    plain = validate(DATASET, model, loaders, epoch=2, log=plain_lines.append, coalesce=4)
    out = tmp_path / "img" / "save"                                         # created by validate
    got = validate(DATASET, model, loaders, epoch=2, log=saved_lines.append, coalesce=4, save_dir=str(out), save_mode=mode)
    assert got == plain and saved_lines == plain_lines and model.training   # coalesce 4: a flush inside each domain
    names, pics = _expected(model, loaders, mode)
    assert len(names) == 12 and sorted(os.listdir(out)) == sorted(names)
    assert [int(n.split("_")[1]) for n in names] == list(range(1, 13)) and names[0][0] == "1" and names[-1][0] == "2"
    differs = 0
    for n, p in zip(names, pics):
        assert np.array_equal(_decode(out / n), p), n
        differs += int((p[..., 0] != p[..., 1]).any())
    assert differs > 0                                                      # something was drawn over the grey image


@pytest.mark.parametrize("dataset,c,k", [("fundus", 3, 2), ("MNMS", 1, 4)])
def test_validate_save_dir_with_planes_and_with_three_part_label_maps(tmp_path, dataset, c, k):
    """the other two prediction forms validate meets: the fundus sigmoid planes, the M&Ms class map (part i = label i + 1)"""
    from networks.unet_model import UNet
    from ustrun import synthetic
    from ustrun.evaluate import validate
    torch.manual_seed(8)
    model = UNet(c, k, base_channels=8).cuda()
    loaders = synthetic.test_loaders(dataset, 1, 2, 2, c, H, seed=9)
    plain = validate(dataset, model, loaders, log=None, coalesce=64)
    for mode in ("mask", "contour"):
        out = tmp_path / mode
        assert validate(dataset, model, loaders, log=None, coalesce=64, save_dir=str(out), save_mode=mode) == plain
        names, pics = _expected(model, loaders, mode, dataset)
        assert len(names) == 4 and sorted(os.listdir(out)) == sorted(names)
        for n, p in zip(names, pics):
            assert np.array_equal(_decode(out / n), p), n


def test_save_mode_is_checked(setup, tmp_path):
    from ustrun.evaluate import validate
    model, loaders = setup
    with pytest.raises(ValueError, match="save_mode"):
        validate(DATASET, model, loaders, log=None, save_dir=str(tmp_path), save_mode="sketch")


def test_script_with_save_img_writes_files(setup, tmp_path):
    import importlib.util
    model, _ = setup
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ust-run_amd")
    spec = importlib.util.spec_from_file_location("ustrun_test_script_gpu", os.path.join(root, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from networks.unet_model import UNet
    torch.manual_seed(6)
    ck = tmp_path / "w.pth"
    torch.save(UNet(n_channels=C, n_classes=K).state_dict(), ck)
    out = tmp_path / "pics"
    args = mod.parser.parse_args(["--dataset", DATASET, "--save_img", "--save_dir", str(out), "--load_path", str(ck), "--test_bs", "2",
                                  "--test_batches", "1", "--domain_num", "2", "--image_size", "64"])
    val, per_domain = mod.main(args)
    files = sorted(os.listdir(out))
    assert len(files) == 4 and [f.split("_")[:2] for f in files] == [["1", "1"], ["1", "2"], ["2", "3"], ["2", "4"]]
    assert all(_decode(out / f).shape == (64, 64, 3) for f in files) and len(per_domain) == 2


def test_util_draw_functions_write_the_batch_paths_pixels(setup, tmp_path):
    from ustrun import render
    from ustrun.evaluate import predict
    from ustrun.trainer import decode_labels
    from utils import util
    model, loaders = setup
    image, label = loaders[1][2]
    image, label = image.cuda(), label.cuda()
    model.eval()
    with torch.no_grad():
        pred, mask = predict(DATASET, model(image)), decode_labels(DATASET, label)
    model.train()
    util.draw_mask_and_save(image[1], pred[1], str(tmp_path / "a" / "m.png"))             # [C,H,W] and an int64 map [H,W]
    assert np.array_equal(_decode(tmp_path / "a" / "m.png"), render.render_mask(image, pred, parts=1)[1].cpu().numpy())
    util.draw_contour_and_save(image[1, 0], pred[1].unsqueeze(0), mask[1], str(tmp_path / "c.png"))      # [H,W] image, [1,H,W] map
    assert np.array_equal(_decode(tmp_path / "c.png"), render.render_contour(image, pred, mask, parts=1)[1].cpu().numpy())
