"""train.py --synthetic 0 end to end on tiny image folders: the readers fill resident pools at the dataset's patch size, the
ResidentLoader's batches (gather, weak and strong augmentation, normalisation: all on the device) drive three SSLTrainer
steps, and validate runs over the resident test splits."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _tree(kind, root, rs):
    from PIL import Image
    from ustrun import datasets as D
    spec = D.SPECS[kind]
    yy, xx = np.mgrid[:64, :64]
    for d in (1, 2):
        listed = []
        for phase, n in (("train", 8), ("test", 2)):
            for i in range(n):
                r = 10 + 2 * i
                disc = (yy - 30 - i) ** 2 + (xx - 34 + i) ** 2 <= r * r
                cup = (yy - 30 - i) ** 2 + (xx - 34 + i) ** 2 <= (r // 2) ** 2
                noise = rs.randint(0, 120, (64, 64, spec["C"])).astype(np.int64)
                img = np.clip(noise + 100 * disc[..., None], 0, 255).astype(np.uint8)
                if kind == "fundus":
                    p = os.path.join(root, "Fundus", f"Domain{d}", phase, "ROIs/image", f"g{i:03d}.png")
                    lab = np.where(cup, 0, np.where(disc, 128, 255)).astype(np.uint8)
                else:
                    p = os.path.join(root, "ProstateSlice", spec["domains"][d], phase, "image", f"{i:02d}_00.png")
                    lab = np.where(disc, 0, 255).astype(np.uint8)
                    img = img[..., 0]
                for path, a in ((p, img), (p.replace("image", "mask"), lab)):
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    Image.fromarray(a).save(path)
                if phase == "train":
                    listed.append(p)
        if kind == "fundus":
            with open(os.path.join(root, "Fundus", f"Domain{d}_train.txt"), "w") as f:
                f.write("\n".join(listed) + "\n")


@pytest.mark.parametrize("kind", ["fundus", "prostate"])
def test_three_steps_and_a_validation_on_image_folders(tmp_path, kind):
    pytest.importorskip("PIL")
    import train as T
    from networks.unet_model import UNet
    from ustrun.evaluate import validate
    from ustrun.trainer import DATASETS, SSLTrainer
    _tree(kind, str(tmp_path), np.random.RandomState(4))
    args = T.parser.parse_args(["--dataset", kind, "--synthetic", "0", "--data_root", str(tmp_path), "--label_bs", "2", "--unlabel_bs", "2",
                                "--lb_domain", "1", "--lb_num", "3", "--domain_num", "2", "--seed", "21"])
    C, H, K = DATASETS[kind][:3]
    dev = torch.device("cuda")
    values = torch.tensor([0.0, 128.0, 255.0] if kind == "fundus" else [0.0, 255.0], device=dev)
    # the 256 levels as synthetic.images forms them: on the CPU (an IEEE division; torch's device kernel multiplies by 1 / 127.5)
    grid = (torch.arange(256, dtype=torch.float32) / 127.5 - 1).to(dev)

    def batches():
        ld = T.make_loaders(args, C, H, dev)
        return [next(ld) for _ in range(3)]
    first, again = batches(), batches()
    for a, b in zip(first, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)                                   # the same seed: the same batches, bit for bit
    for lx, ly, ux, us, uy in first:
        assert lx.shape == ux.shape == us.shape == (2, C, H, H) and lx.dtype == torch.float32 and lx.is_cuda
        assert ly.shape == uy.shape == (2, H, H) and ly.dtype == torch.float32
        for name, x in (("lb_x_w", lx), ("ulb_x_w", ux), ("ulb_x_s", us)):
            assert bool(torch.isin(x, grid).all()), name + " leaves the grid k / 127.5 - 1"
        assert not torch.equal(us, ux)                                 # the strong view is not the weak view
        assert bool(torch.isin(ly, values).all()) and bool(torch.isin(uy, values).all())
    assert not torch.equal(first[0][2], first[1][2])

    torch.manual_seed(5)
    stu, tea = UNet(C, K, base_channels=8).cuda(), UNet(C, K, base_channels=8).cuda()
    before = [p.detach().clone() for p in stu.parameters()]
    trn = SSLTrainer(kind, stu, tea, max_iterations=300, patch_size=H, num_eval_iter=3, fft="device")
    for i, b in enumerate(first):
        trn.step(*b, epoch_start=(i == 0))
        s = trn.scalars()
        assert all(np.isfinite(s[k]) for k in ("loss", "sup", "ul", "lu", "s")), s
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, stu.parameters()))

    loaders = T.make_test_loaders(args, C, H, dev)
    assert len(loaders) == 2 and [len(l) for l in loaders] == [2, 2]
    val, per_domain = validate(kind, tea, loaders, epoch=1, log=None)
    assert len(per_domain) == 2 and all(np.isfinite(v) for v in val) and all(np.isfinite(v) for d in per_domain for v in d)
