"""The tensor arithmetic of the reference's dataloaders/utils.py on the device: `post_processing` (:193-204, ustrun_post_process)
and `post_processing_volume` (the same lines on a volume, ustrun_post_process_3d), `cross_entropy2d` (:128-144, ustrun_ce_map), `get_iou` / `get_dice` (:150-188, from one confusion matrix per image, ustrun_confusion)
and the colour decoders (:78-120, ustrun_colorize), beside the host helpers `encode_segmap`, `lr_poly` and `untransform`.  There is no
CPU fallback for the device functions: without the library or a HIP device the call raises.

Conventions: a numpy array in gives numpy float64 out, a device tensor in gives a device tensor out.  Functions that return a Python
float in the reference wait for their result here too."""
import numpy as np
import torch

from ustrun import functional as F
from utils.metrics import confusion_counts


def post_processing(prediction):
    """One 2-D binary plane (numpy array or tensor on any device; non-zero = foreground) -> the plane with its holes filled and
    every 8-connected component below a fifth of the filled foreground removed.  A numpy input gives a bool numpy array, as the
    reference returns; a tensor gives a tensor of its device and dtype."""
    is_np = not torch.is_tensor(prediction)
    t = torch.from_numpy(np.ascontiguousarray(prediction)) if is_np else prediction
    if t.dim() != 2:
        raise ValueError("post_processing takes one 2-D plane, got shape %r" % (tuple(t.shape),))
    out = F.post_process((t != 0).to(device="cuda", dtype=torch.float32)[None, None])[0, 0]
    if is_np:
        return out.cpu().numpy().astype(bool)
    return out.to(device=t.device, dtype=t.dtype)


def post_processing_volume(prediction):
    """One 3-D binary volume [D,H,W] (numpy array or tensor on any device; non-zero = foreground) -> what the reference's
    post_processing computes when handed the volume, its scipy / skimage calls being n-dimensional: cavities filled (background
    that no path of face steps leads from to a face of the volume), every 26-connected component below a fifth of the filled
    foreground removed (ustrun_post_process_3d).  Conventions as `post_processing`, which keeps refusing anything but a plane:
    numpy in gives a bool numpy array, a tensor a tensor of its device and dtype."""
    is_np = not torch.is_tensor(prediction)
    t = torch.from_numpy(np.ascontiguousarray(prediction)) if is_np else prediction
    if t.dim() != 3:
        raise ValueError("post_processing_volume takes one 3-D volume, got shape %r" % (tuple(t.shape),))
    out = F.post_process_3d((t != 0).to(device="cuda", dtype=torch.float32)[None, None])[0, 0]
    if is_np:
        return out.cpu().numpy().astype(bool)
    return out.to(device=t.device, dtype=t.dtype)


def untransform(img, lt):
    """Undo the [-1, 1] image scaling and the / 128 label scaling (dataloaders/utils.py:10-13)."""
    return (img + 1) * 127.5, lt * 128


def lr_poly(base_lr, iter_, max_iter=100, power=0.9):
    """Polynomial learning-rate decay (dataloaders/utils.py:146-147)."""
    return base_lr * ((1 - float(iter_) / max_iter) ** power)


# The 19 Cityscapes train ids in order, with the colours of the cityscapesScripts label table -- except "sky", which the reference's
# table (dataloaders/utils.py:38) has as (0, 130, 180) where cityscapesScripts has (70, 130, 180); a drop-in keeps the reference's.
_CITYSCAPES = (("road", (128, 64, 128)), ("sidewalk", (244, 35, 232)), ("building", (70, 70, 70)), ("wall", (102, 102, 156)),
               ("fence", (190, 153, 153)), ("pole", (153, 153, 153)), ("traffic light", (250, 170, 30)), ("traffic sign", (220, 220, 0)),
               ("vegetation", (107, 142, 35)), ("terrain", (152, 251, 152)), ("sky", (0, 130, 180)), ("person", (220, 20, 60)),
               ("rider", (255, 0, 0)), ("car", (0, 0, 142)), ("truck", (0, 0, 70)), ("bus", (0, 60, 100)), ("train", (0, 80, 100)),
               ("motorcycle", (0, 0, 230)), ("bicycle", (119, 11, 32)))


def get_cityscapes_labels():
    """[19,3] integer array: the colour of every Cityscapes train id."""
    return np.array([rgb for _, rgb in _CITYSCAPES])


def get_pascal_labels():
    """[21,3] integer array: the PASCAL VOC colour map.  Class i spreads its bits over the channels, bit 3j + c of i becoming bit
    7 - j of channel c (the VOC devkit's bit-interleave)."""
    out = np.zeros((21, 3), dtype=int)
    for i in range(21):
        for j in range(8):
            for c in range(3):
                out[i, c] |= ((i >> (3 * j + c)) & 1) << (7 - j)
    return out


def encode_segmap(mask):
    """A PASCAL colour image [M,N,3] -> the class map [M,N] (int): the index of the pixel's colour in `get_pascal_labels`, 0 for a
    colour that is not in it (dataloaders/utils.py:61-75).  Host numpy."""
    mask = np.asarray(mask).astype(int)
    key = lambda a: (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]
    colours = key(get_pascal_labels())
    order = np.argsort(colours)
    is_byte = np.all((mask >= 0) & (mask <= 255), axis=-1)
    keys = np.where(is_byte, key(mask), -1)
    at = np.minimum(np.searchsorted(colours[order], keys), len(colours) - 1)
    return np.where(colours[order][at] == keys, order[at], 0).astype(int)


def _palette(dataset):
    if dataset == "pascal":
        return get_pascal_labels().astype(np.uint8)
    if dataset == "cityscapes":
        return get_cityscapes_labels().astype(np.uint8)
    raise NotImplementedError


def _decode(label_masks, dataset):
    """[N,...] labels -> (float32 device tensor [N,3,...], the input was an integer numpy array)"""
    pal = _palette(dataset)
    if torch.is_tensor(label_masks) and label_masks.is_cuda:
        t = label_masks if label_masks.dtype in (torch.int64, torch.float32) else (label_masks.float() if label_masks.is_floating_point() else label_masks.long())
        return F.colorize(t, pal), False
    a = np.asarray(label_masks.cpu() if torch.is_tensor(label_masks) else label_masks)
    exact = a.dtype.kind in "iub"
    return F.colorize(torch.from_numpy(np.ascontiguousarray(a.astype(np.int64 if exact else np.float32))).cuda(), pal), exact


def _to_float64(rgb, exact):
    """the device's float32 c / 255 as the float64 quotient the reference returns: for integer labels c = rint(255 v) exactly"""
    v = rgb.cpu().numpy().astype(np.float64)
    return np.rint(v * 255.0) / 255.0 if exact else v


def decode_segmap(label_mask, dataset, plot=False):
    """One class map [M,N] -> the colour image [M,N,3] in [0,1] (dataloaders/utils.py:86-120): numpy in gives float64 numpy, a
    device tensor gives a float32 device tensor.  A label outside the palette keeps label / 255 in all three channels, as the
    reference's copies do."""
    rgb, exact = _decode(label_mask[None], dataset)
    rgb = rgb[0].permute(1, 2, 0)
    if not (torch.is_tensor(label_mask) and label_mask.is_cuda):
        rgb = _to_float64(rgb, exact)
    if not plot:
        return rgb
    import matplotlib.pyplot as plt
    plt.imshow(rgb if isinstance(rgb, np.ndarray) else rgb.cpu().numpy())
    plt.show()


def decode_seg_map_sequence(label_masks, dataset='pascal'):
    """A batch of class maps [B,M,N] -> [B,3,M,N] colour images: a float64 CPU tensor for host input, as the reference returns
    (dataloaders/utils.py:78-84), a float32 device tensor for a device tensor."""
    rgb, exact = _decode(label_masks, dataset)
    if torch.is_tensor(label_masks) and label_masks.is_cuda:
        return rgb
    return torch.from_numpy(_to_float64(rgb, exact))


def _class_weights(weight, device):
    if weight is None:
        return None
    if torch.is_tensor(weight):
        return weight.to(device=device, dtype=torch.float32)
    return torch.from_numpy(np.array(weight, dtype=np.float32)).to(device)


def cross_entropy2d(logit, target, ignore_index=255, weight=None, size_average=True, batch_average=True):
    """sum over the pixels with target != ignore_index of weight[t] * nll, divided by H*W (size_average) and by N (batch_average)
    (dataloaders/utils.py:128-144).  weight: a list, an array or a tensor of one value per class.  A device scalar, differentiable
    in `logit`; nothing on the host waits."""
    n, c, h, w = logit.size()
    scale = 1.0 / ((h * w if size_average else 1) * (n if batch_average else 1))
    return F.ce_map(logit, target.long(), weight=_class_weights(weight, logit.device), ignore_index=ignore_index, scale=scale)


def get_iou(pred, gt, n_classes=21):
    """The sum over the images of the mean, over the classes present in pred or gt, of |pred == j & gt == j| / |pred == j | gt == j|
    -- a Python float, from one confusion matrix per image counted on the device.  ValueError if a label is outside [0, n_classes).

    This is the IoU the reference's get_iou (dataloaders/utils.py:150-176) means, NOT what it returns under today's torch: there
    `(pred == j) + (gt == j)` is a logical OR of bool tensors, so `match == 2` never holds and the function returns 0.0 for every
    input."""
    c = confusion_counts(pred, gt, n_classes, "get_iou").astype(np.float64)
    total = 0.0
    for m in c:
        inter = np.diag(m)
        union = m.sum(0) + m.sum(1) - inter
        present = union > 0
        total += float((inter[present] / union[present]).sum() / present.sum())
    return total


GET_DICE_CLASSES = 32


def get_dice(pred, gt):
    """sum over the images of 2 sum p g / (sum p^2 + sum g^2) on the integer labels (dataloaders/utils.py:178-188), a Python
    float, from one confusion matrix per image: sum p g = sum_{a,b} a b C[a][b], sum p^2 = sum_b b^2 col_b, sum g^2 = sum_a a^2
    row_a, exact for any labels in [0, 32) and not only for binary masks.  ValueError for a label outside that range;
    ZeroDivisionError for an image where both maps are all zero, as in the reference."""
    c = confusion_counts(pred, gt, GET_DICE_CLASSES, "get_dice")
    v = np.arange(GET_DICE_CLASSES, dtype=np.int64)
    total = 0.0
    for m in c:
        pg = int(v @ m @ v)
        pp, gg = int((v * v) @ m.sum(0)), int((v * v) @ m.sum(1))
        total += 2.0 * pg / (pp + gg)
    return total
