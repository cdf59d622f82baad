"""Image-folder data path of pre-training (`--data_set IMNET | image_folder | tiny_IMNET`): the reference's
`ImageFolder(args.data_path, transform=DataAugmentationForBEiT(args))` (datasets.py:31-139, dataset_folder.py) with the
augmentation itself moved onto the GPU.

    DataLoader worker: PIL decode + convert('RGB') -> draw the augmentation parameters (same random sources, same order
                       as the reference's transforms) -> block-wise mask
    collate:           pack the batch's uint8 HWC pixels and one uvit_augment_desc per sample (pinned by the loader)
    DevicePrefetcher:  upload on its side stream, uvit_op_augment_batch -> normalized fp32 (B, 3, S, S)

The device produces the bytes Pillow + torchvision produce for the same parameters (csrc/augment.hip; restated in NumPy by
tests/augment_util.py).  torchvision is not a dependency: the few pieces of its geometry the transforms use are restated
below, each citing the torchvision function it follows.
"""
import math
import os
import random

import numpy as np
import torch

from .masking_generator import MaskingGenerator

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")   # dataset_folder.py:184
IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # timm.data.constants
IMAGENET_INCEPTION_MEAN, IMAGENET_INCEPTION_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
FOLDER_DATA_SETS = ("IMNET", "image_folder", "tiny_IMNET")

# filter ids = PIL.Image.Resampling (include/uvit.h UVIT_AUG_*); jitter op ids = ColorJitter's fn_idx
LANCZOS, BILINEAR, BICUBIC, HAMMING = 1, 2, 3, 5
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2

# uvit_augment_desc (include/uvit.h) as a NumPy record: the collate function fills an array of these in place
AUG_DESC_DTYPE = np.dtype([("offset", "<i8")] +
                          [(n, "<i4") for n in ("h", "w", "flip", "crop_x", "crop_y", "crop_w", "crop_h", "resize_w", "resize_h",
                                                "win_x", "win_y", "filter", "n_jitter")] +
                          [("jitter_op", "<i4", (3,)), ("jitter_factor", "<f4", (3,)), ("reserved", "<i4")], align=True)


def pil_interp(method):
    """transforms.py:53-62 of the reference (anything unknown is bilinear)."""
    return {"bicubic": BICUBIC, "lanczos": LANCZOS, "hamming": HAMMING}.get(method, BILINEAR)


# ---------------------------------------------------------------------------------------------------------------- folder scan
def find_classes(root):
    """dataset_folder.py:139-153: the sub-directories of root, sorted; class index = position."""
    classes = sorted(d.name for d in os.scandir(root) if d.is_dir())
    return classes, {c: i for i, c in enumerate(classes)}


def make_dataset(root, class_to_idx, extensions=IMG_EXTENSIONS):
    """dataset_folder.py:38-66: (path, class index) for every file with an image extension, classes in sorted order,
    os.walk(followlinks=True) sorted, file names sorted within a directory."""
    out = []
    root = os.path.expanduser(root)
    for target_class in sorted(class_to_idx):
        target_dir = os.path.join(root, target_class)
        if not os.path.isdir(target_dir):
            continue
        for dirpath, _, fnames in sorted(os.walk(target_dir, followlinks=True)):
            for fname in sorted(fnames):
                if fname.lower().endswith(extensions):
                    out.append((os.path.join(dirpath, fname), class_to_idx[target_class]))
    return out


def pil_loader(path):
    """dataset_folder.py:187-191: PIL decode, convert('RGB') -> (H, W, 3) uint8."""
    from PIL import Image
    with open(path, "rb") as f:
        return np.asarray(Image.open(f).convert("RGB"))


# ----------------------------------------------------------------------------------------------- torchvision geometry, restated
def resize_short_side(h, w, size):
    """torchvision.transforms.functional._compute_resized_output_size for Resize(int): the short side becomes `size`, the long
    side int(size * long / short).  Returns (new_h, new_w)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


def center_crop_origin(h, w, size):
    """torchvision.transforms.functional.center_crop: (top, left) of the size x size crop of an h x w image.  A side shorter than
    `size` is first zero-padded by (size - side) // 2 before (the origin is then minus that), a longer side is cropped at
    int(round((side - size) / 2.0)) (Python's round: half to even)."""
    def origin(side):
        return -((size - side) // 2) if size > side else int(round((side - size) / 2.0))
    return origin(h), origin(w)


def rrc_params_torch(h, w, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision.transforms.RandomResizedCrop.get_params (torch RNG): (i, j, crop_h, crop_w)."""
    area = h * w
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        cw = int(round(math.sqrt(target_area * aspect_ratio)))
        ch = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < cw <= w and 0 < ch <= h:
            i = torch.randint(0, h - ch + 1, size=(1,)).item()
            j = torch.randint(0, w - cw + 1, size=(1,)).item()
            return i, j, ch, cw
    in_ratio = float(w) / float(h)
    if in_ratio < min(ratio):
        cw, ch = w, int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        ch, cw = h, int(round(h * max(ratio)))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def rrc_params_two_pic(h, w, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCropAndInterpolationWithTwoPic.get_params (reference transforms.py:109-145, Python `random`):
    (i, j, crop_h, crop_w) of an image of width w and height h."""
    area = w * h
    for _ in range(10):
        target_area = random.uniform(*scale) * area
        log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
        aspect_ratio = math.exp(random.uniform(*log_ratio))
        cw = int(round(math.sqrt(target_area * aspect_ratio)))
        ch = int(round(math.sqrt(target_area / aspect_ratio)))
        if cw <= w and ch <= h:
            i = random.randint(0, h - ch)
            j = random.randint(0, w - cw)
            return i, j, ch, cw
    in_ratio = w / h
    if in_ratio < min(ratio):
        cw = w
        ch = int(round(cw / min(ratio)))
    elif in_ratio > max(ratio):
        ch = h
        cw = int(round(ch * max(ratio)))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def color_jitter_params(b=0.4, c=0.4, s=0.4):
    """torchvision ColorJitter(b, c, s).get_params: order = randperm(4) without the hue step (hue 0 is None), then one
    uniform factor per step in [1 - v, 1 + v].  Returns [(op, factor)] in application order."""
    fn_idx = torch.randperm(4)
    f = [float(torch.empty(1).uniform_(max(0.0, 1 - v), 1 + v)) for v in (b, c, s)]
    return [(int(i), f[int(i)]) for i in fn_idx if int(i) < 3]


# --------------------------------------------------------------------------------------------------------------- augmentation
class BEiTAugment:
    """DataAugmentationForBEiT (reference datasets.py:31-117) split in two: `__call__` draws one sample's parameters on the host
    (a uvit_augment_desc record) in the reference's order of random draws; the pixels are produced on the device.

    aug_level -1 (default): ColorJitter(0.4, 0.4, 0.4) -> flip -> RandomResizedCropAndInterpolationWithTwoPic(input_size,
                            train_interpolation; 'random' = bilinear or bicubic per sample)
              0: CenterCrop          1: Resize(int(S / .875), bicubic) -> CenterCrop       2: flip -> level 1
              3: flip -> RandomResizedCrop(S, bicubic)                                      4: ColorJitter -> level 3
    The second picture of the d-VAE tokenizer (second_input_size) is not built: the cyclical pre-training never sets it."""

    def __init__(self, input_size, aug_level=-1, train_interpolation="bicubic", imagenet_default_mean_and_std=False):
        if aug_level not in (-1, 0, 1, 2, 3, 4):
            aug_level = -1             # the reference's `else` branch
        self.size, self.aug_level = int(input_size), aug_level
        self.interpolation = (BILINEAR, BICUBIC) if train_interpolation == "random" else pil_interp(train_interpolation)
        self.mean = IMAGENET_DEFAULT_MEAN if imagenet_default_mean_and_std else IMAGENET_INCEPTION_MEAN
        self.std = IMAGENET_DEFAULT_STD if imagenet_default_mean_and_std else IMAGENET_INCEPTION_STD

    def __repr__(self):
        return f"BEiTAugment(size={self.size}, aug_level={self.aug_level}, interpolation={self.interpolation}, mean={self.mean}, std={self.std})"

    def __call__(self, h, w):
        """Parameters of one h x w image: an AUG_DESC_DTYPE record (offset filled in by the collate function)."""
        S, lvl = self.size, self.aug_level
        d = np.zeros((), AUG_DESC_DTYPE)
        d["h"], d["w"] = h, w
        jit = color_jitter_params() if lvl in (-1, 4) else []
        flip = lvl in (-1, 2, 3, 4) and bool(torch.rand(1) < 0.5)
        flt = BICUBIC
        if lvl == -1:
            i, j, ch, cw = rrc_params_two_pic(h, w)
            flt = random.choice(self.interpolation) if isinstance(self.interpolation, tuple) else self.interpolation
            rh, rw, wy, wx = S, S, 0, 0
        elif lvl in (3, 4):
            i, j, ch, cw = rrc_params_torch(h, w)
            rh, rw, wy, wx = S, S, 0, 0
        else:
            i, j, ch, cw = 0, 0, h, w
            rh, rw = (h, w) if lvl == 0 else resize_short_side(h, w, int(S / .875))
            wy, wx = center_crop_origin(rh, rw, S)
        d["flip"], d["filter"] = int(flip), flt
        d["crop_y"], d["crop_x"], d["crop_h"], d["crop_w"] = i, j, ch, cw
        d["resize_h"], d["resize_w"], d["win_y"], d["win_x"] = rh, rw, wy, wx
        d["n_jitter"] = len(jit)
        for k, (op, f) in enumerate(jit):
            d["jitter_op"][k], d["jitter_factor"][k] = op, f
        return d


class PackedBatch:
    """One loader batch before augmentation: every image's pixels back to back (uint8 HWC), one uvit_augment_desc per sample
    (`desc`, uint8 view of B records), the (B, gh, gw) masks and the labels.  `pin_memory()` is what DataLoader(pin_memory=True)
    calls on it."""

    def __init__(self, pixels, desc, mask, labels, size, mean, std):
        self.pixels, self.desc, self.mask, self.labels = pixels, desc, mask, labels
        self.size, self.mean, self.std = size, mean, std

    def __len__(self):
        return self.mask.shape[0]

    def pin_memory(self):
        return PackedBatch(self.pixels.pin_memory(), self.desc.pin_memory(), self.mask.pin_memory(), self.labels.pin_memory(),
                           self.size, self.mean, self.std)

    def records(self):
        """The descriptors as an AUG_DESC_DTYPE array (a view of `desc`)."""
        return self.desc.numpy().view(AUG_DESC_DTYPE)


def collate_packed(batch):
    """[((pixels (h, w, 3) uint8, desc record, mask), label)] -> PackedBatch; fills each descriptor's byte offset."""
    items = [b[0] for b in batch]
    desc = np.stack([it[1] for it in items]).astype(AUG_DESC_DTYPE)
    sizes = [it[0].size for it in items]
    desc["offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    pixels = torch.from_numpy(np.concatenate([np.ascontiguousarray(it[0]).reshape(-1) for it in items]))
    mask = torch.from_numpy(np.stack([it[2] for it in items]))
    labels = torch.as_tensor([b[1] for b in batch], dtype=torch.int64)
    first = batch[0][0]
    return PackedBatch(pixels, torch.from_numpy(desc.view(np.uint8).reshape(-1)), mask, labels, first[3], first[4], first[5])


class ImageFolderPretrain(torch.utils.data.Dataset):
    """ImageFolder(data_path, transform=DataAugmentationForBEiT(args)) of the reference (datasets.py:131-139) with the pixel work
    left for the device: item = ((pixels, desc, mask, size, mean, std), class index)."""

    def __init__(self, root, augment, window_size, num_masking_patches, max_num_patches=None, min_num_patches=16):
        self.root, self.augment = root, augment
        self.classes, self.class_to_idx = find_classes(root)
        self.samples = make_dataset(root, self.class_to_idx)
        if not self.samples:
            raise RuntimeError(f"Found 0 files in subfolders of: {root}\nSupported extensions are: {','.join(IMG_EXTENSIONS)}")
        self.targets = [s[1] for s in self.samples]
        self.masks = MaskingGenerator(tuple(window_size), num_masking_patches, min_num_patches=min_num_patches,
                                      max_num_patches=max_num_patches)
        # the reference's generator draws from the global `random` stream (masking_generator.py:54-66), right after the crop
        # parameters; DataLoader seeds that stream per worker
        self.masks.rng = random

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        while True:     # dataset_folder.py:165-172: an unreadable file is replaced by a random other one
            try:
                path, target = self.samples[index]
                img = pil_loader(path)
                break
            except Exception as e:  # noqa: BLE001 -- the reference catches everything here
                print(e)
                index = random.randint(0, len(self.samples) - 1)
        desc = self.augment(img.shape[0], img.shape[1])
        a = self.augment
        return (img, desc, self.masks(), a.size, a.mean, a.std), target


class PerturbationSequences(torch.utils.data.Dataset):
    """One perturbation of a CIFAR-100-P style data set: a `.npy` of shape (N, F, H, W, 3) uint8, N sequences of F frames, the file
    the reference's build_p_dataset reads (uncertainty_evaluations.py:784-799).  It is opened with mmap_mode="r"; one item is one
    sequence, ((pixels (F, H, W, 3), F descriptors, size, mean, std), 0), for `collate_sequences`.  `augment` is the evaluation
    pipeline of the classifier (BEiTAugment(input_size, 1, "bicubic", ...): bicubic resize of the short side + centre crop on the
    device, with the mean and std the head was trained with), not the reference's process_raw_data, which always normalises with the
    inception constants and then applies `* 2 - 1` once more."""

    def __init__(self, npy_path, augment):
        self.path, self.augment = npy_path, augment
        self.data = np.load(npy_path, mmap_mode="r")
        if self.data.ndim != 5 or self.data.shape[-1] != 3 or self.data.dtype != np.uint8:
            raise ValueError(f"{npy_path}: expected a uint8 array of shape (N, F, H, W, 3), found {self.data.dtype} {self.data.shape}")
        if self.data.shape[1] < 2:
            raise ValueError(f"{npy_path}: a sequence needs at least two frames")
        self.frames = int(self.data.shape[1])
        d = augment(int(self.data.shape[2]), int(self.data.shape[3]))       # level 1 draws nothing: every frame has these parameters
        self._desc = np.repeat(d.reshape(1), self.frames).astype(AUG_DESC_DTYPE)

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, index):
        a = self.augment
        return (np.ascontiguousarray(self.data[index]), self._desc, a.size, a.mean, a.std), 0


def collate_sequences(batch):
    """[((pixels (F, H, W, 3) uint8, F desc records, size, mean, std), 0)] -> PackedBatch of V F images, sequence-major: the frames of
    a sequence stay adjacent and in frame order.  Labels are 0 and the mask is (V F, 1) zeros: the probe's forward takes none."""
    items = [b[0] for b in batch]
    desc = np.concatenate([it[1] for it in items]).astype(AUG_DESC_DTYPE)
    sizes = np.concatenate([[it[0][f].size for f in range(it[0].shape[0])] for it in items])
    desc["offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    pixels = torch.from_numpy(np.concatenate([it[0].reshape(-1) for it in items]))
    n = desc.shape[0]
    first = items[0]
    return PackedBatch(pixels, torch.from_numpy(desc.view(np.uint8).reshape(-1)), torch.zeros(n, 1, dtype=torch.int64),
                       torch.zeros(n, dtype=torch.int64), first[2], first[3], first[4])


def build_pretraining_dataset(args):
    """build_beit_pretraining_dataset (reference datasets.py:131-139) for the folder data sets."""
    if args.data_set in ("CIFAR10", "CIFAR100"):
        raise NotImplementedError(f"--data_set {args.data_set} needs torchvision's CIFAR archive format, which is not available here; "
                                  "use an image folder (IMNET / image_folder / tiny_IMNET) or SYNTHETIC")
    if args.data_set not in FOLDER_DATA_SETS:
        raise ValueError(args.data_set)
    aug = BEiTAugment(args.input_size, args.aug_level, args.train_interpolation, args.imagenet_default_mean_and_std)
    print("Data Aug = %s" % aug)
    return ImageFolderPretrain(args.data_path, aug, args.window_size, args.num_mask_patches,
                               max_num_patches=args.max_mask_patches_per_block, min_num_patches=args.min_mask_patches_per_block)
