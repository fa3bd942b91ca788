"""Frame-folder video datasets and their HBM-resident preload.

The reference reads its real clips from folders of JPEG frames through six near-identical ``Dataset`` classes
(distill_utils/dataset.py: ``UCF101`` :146-249, ``HMDB51`` :251-351, ``miniUCF101`` :353-467, ``miniHMDB51`` :469-568,
``Kinetics400`` :79-144, ``SSv2`` :841-895) and, under ``--preload``, stacks every item into one host tensor that ``get_images`` then slices and
copies to the GPU per class and step (distill_baseline.py:36-45, 84-90; 7.7 GB of PCIe traffic per step at config 2).

Here one class, ``FrameFolderVideos``, covers the six (a ``spec`` says where the index file is and how frames are
picked), with the reference's item semantics — including the ORDER in which the global ``numpy.random`` / ``random`` /
``torch`` generators are consumed, so a seeded run picks the same frames, flips and crops — and ``preload`` puts the
whole split into HBM once: JPEG decode on host threads (PIL releases the GIL), uint8 frames through pinned staging,
``vd_frames_normalize`` (HWC uint8 -> CHW fp32, ``(v/255 - mean)/std``, the arithmetic of torchvision's
``ToTensor`` + ``Normalize``) on the device.  A 112x112x16 split of miniUCF101 (4662 clips) is 11.2 GB of fp32 clips:
resident, and the per-step gather is an index_select on the device (``distill.RealPool``).

``StillFrameVideos`` covers the reference's still-image variants (``staticHMDB51`` :570-650, ``staticUCF101`` :652-736,
``staticUCF50`` :738-839, ``singleKinetics400`` :18-77, ``singleSSv2`` :897-947): one frame of a video, repeated into a
"boring" clip or handed out as an image.  They feed the reference's static-memory learning stage, which is off the hot
path, so they are host-side only (no preload kernel of their own: an item is a clip or an image like any other).

``preload`` freezes one draw per item.  Where the reference draws per READ -- a test item's start frame on every one of
``epoch('test')``'s three passes, the flip of every item -- ``ResidentVideos`` keeps whole videos in HBM instead (every frame
decoded once, uint8) and ``ResidentClipLoader`` draws each batch's frames / flips / crops on the host, in the DataLoader's
generator order, and lets ``vd_clips_sample`` gather, mirror, crop and normalise them: the host loader's clips, bit for bit,
without a JPEG decode per read.
"""
from __future__ import annotations

import csv
import json
import os
import os.path as osp
import random
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data as tdata

NUM_FRAMES = 16          # distill_utils/dataset.py:15
FRAME_GAP = 4            # distill_utils/dataset.py:16
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


@dataclass(frozen=True)
class FolderSpec:
    """How one dataset family is laid out on disk and how a clip's frames are chosen."""
    index: str                       # 'csv-splits' (UCF/HMDB), 'csv-kinetics', 'json-ssv2'
    index_file: str                  # file name under the dataset root ('{split}' is substituted)
    frames_root: str                 # sub-directory holding one folder per video
    pick: str                        # 'window' (random start + stride), 'segments' (one frame per 1/16), 'all'


SPECS = {
    'UCF101': FolderSpec('csv-splits', 'ucf101_splits1.csv', 'jpegs_112', 'window'),
    'HMDB51': FolderSpec('csv-splits', 'hmdb51_splits.csv', 'jpegs_112', 'window'),
    'miniUCF101': FolderSpec('csv-splits', 'ucf50_splits1.csv', 'jpegs_112', 'window'),
    'miniHMDB51': FolderSpec('csv-splits', 'hmdb25_splits.csv', 'jpegs_112', 'window'),          # distill_utils/dataset.py:469-568
    'Kinetics400': FolderSpec('csv-kinetics', '{split}.csv', '{split}', 'all'),
    'SSv2': FolderSpec('json-ssv2', 'annot_{split}.json', 'frame', 'all'),
}


class FrameTransform:
    """``ToTensor`` + ``Normalize`` and, when the target size is not the stored 112x112, ``Resize((100, 80))`` +
    ``RandomCrop(im_size)`` in front (utils.py:164-174 and its twins).  torchvision is not needed: a PIL image goes
    through PIL's own bilinear resize (what torchvision calls for PIL inputs), a crop whose offsets are drawn as
    ``RandomCrop.get_params`` draws them (``torch.randint`` for the row, then the column; none when nothing is cut), and
    ``uint8/255`` followed by ``(x - mean)/std`` in fp32."""

    def __init__(self, im_size: Tuple[int, int], mean=IMAGENET_MEAN, std=IMAGENET_STD, stored=(112, 112)):
        self.im_size = tuple(im_size)
        self.resize = None if self.im_size == tuple(stored) else (100, 80)
        self.mean = torch.tensor(mean, dtype=torch.float32)
        self.std = torch.tensor(std, dtype=torch.float32)

    def draw(self, height: int, width: int):
        """The random part of one call: the crop origin (None when the transform has no crop)."""
        if self.resize is None:
            return None
        h, w = self.resize
        th, tw = self.im_size
        if h < th or w < tw:
            raise ValueError("Required crop size %s is larger than input image size %s" % ((th, tw), (h, w)))
        if (h, w) == (th, tw):
            return (0, 0)
        i = int(torch.randint(0, h - th + 1, size=(1,)).item())
        j = int(torch.randint(0, w - tw + 1, size=(1,)).item())
        return (i, j)

    def pixels(self, image, crop) -> np.ndarray:
        """PIL image -> (H, W, 3) uint8 after resize / crop."""
        from PIL import Image
        if image.mode != 'RGB':
            image = image.convert('RGB')
        if self.resize is not None:
            image = image.resize((self.resize[1], self.resize[0]), Image.BILINEAR)
            i, j = crop
            image = image.crop((j, i, j + self.im_size[1], i + self.im_size[0]))
        return np.asarray(image, dtype=np.uint8)

    def stored_pixels(self, image) -> np.ndarray:
        """PIL image -> (Hs, Ws, 3) uint8 after the deterministic part only (RGB conversion, resize): what ``ResidentVideos``
        keeps per frame.  The flip and the crop of a read are applied to it on the device."""
        from PIL import Image
        if image.mode != 'RGB':
            image = image.convert('RGB')
        if self.resize is not None:
            image = image.resize((self.resize[1], self.resize[0]), Image.BILINEAR)
        return np.asarray(image, dtype=np.uint8)

    def normalise(self, u8: torch.Tensor) -> torch.Tensor:
        """(..., H, W, 3) uint8 -> (..., 3, H, W) fp32; the host-side twin of ``vd_frames_normalize``."""
        x = u8.movedim(-1, -3).to(torch.float32).div(255)
        return x.sub_(self.mean.view(3, 1, 1)).div_(self.std.view(3, 1, 1))

    def __call__(self, image) -> torch.Tensor:
        crop = self.draw(image.height, image.width)
        return self.normalise(torch.from_numpy(self.pixels(image, crop).copy()))


@dataclass
class ClipDraw:
    """Everything random about one item, drawn up front so that the file reads can run on worker threads."""
    files: List[str]
    flip: bool
    crops: List[Optional[Tuple[int, int]]]


class FrameFolderVideos(tdata.Dataset):
    """``dataset[i] -> (clip (T, 3, H, W) fp32, label)`` over a folder of per-video frame directories.

    ``family`` picks the layout (``SPECS``); ``split`` is 'train' / 'test' ('val' for Kinetics400 / SSv2).  Labels
    are positions in the sorted set of label strings of THIS split, ``labels`` / ``targets`` list them per item, and the
    start frame of a training item is drawn once and kept (``self.start``), as in the reference."""

    def __init__(self, family: str, path: str, split: str, transform: Optional[FrameTransform] = None, sample: str = 'random'):
        if family not in SPECS:
            raise ValueError("unknown dataset family: %s" % family)
        self.family, self.spec, self.split, self.sample = family, SPECS[family], split, sample
        self.transform = transform if transform is not None else FrameTransform((112, 112))
        self.root = path
        names, label_strs, self.skipped = self._read_index(path, split)
        self.video_dirs = names
        self.label_strs = label_strs
        self.class_strs = sorted(set(label_strs))
        self.class_2_idx = {s: i for i, s in enumerate(self.class_strs)}
        self.labels = [self.class_2_idx[s] for s in label_strs]
        self.targets = self.labels
        self.start = [-1] * len(self.video_dirs)

    # -- index files -----------------------------------------------------------------------------------------------------
    def _expected_frames(self, path: str) -> int:
        tail = path.split("/")[-1]
        return 8 if tail in ("kinetics_64x64x8", "SSv2_64x8") else NUM_FRAMES       # dataset.py:81-84, 843-846

    def _read_index(self, path: str, split: str):
        spec = self.spec
        dirs, labels, skipped = [], [], 0
        if spec.index == 'csv-splits':
            frames_root = osp.join(path, spec.frames_root)
            with open(osp.join(path, spec.index_file)) as fp:
                for row in csv.DictReader(fp):
                    if row["split"] != split:
                        continue
                    dirs.append(osp.join(frames_root, row["folder_name"]))
                    labels.append(row["label"])
            return dirs, labels, 0
        want = self._expected_frames(path)

        def usable(d):
            return osp.exists(d) and len(os.listdir(d)) == want
        if spec.index == 'csv-kinetics':
            csv_split = "validate" if split == "val" else split
            with open(osp.join(path, "%s.csv" % csv_split)) as fp:
                for row in csv.DictReader(fp):
                    if row["split"] != csv_split:
                        raise AssertionError("row of split %r in %s.csv" % (row["split"], csv_split))
                    name = "%s_%06d_%06d" % (row["youtube_id"], int(row["time_start"]), int(row["time_end"]))
                    d = osp.join(path, split, name)
                    if not usable(d):
                        d = osp.join(path, "replacement", name)
                    if not usable(d):
                        skipped += 1
                        continue
                    dirs.append(d)
                    labels.append(row["label"])
            return dirs, labels, skipped
        with open(osp.join(path, spec.index_file.format(split=split))) as fp:
            for item in json.load(fp):
                d = osp.join(path, spec.frames_root, item['id'])
                if not usable(d):
                    skipped += 1
                    continue
                dirs.append(d)
                labels.append(item["class"])
        return dirs, labels, skipped

    def __len__(self) -> int:
        return len(self.video_dirs)

    # -- one item: the draws, then the reads -----------------------------------------------------------------------------
    def draw(self, index: int) -> ClipDraw:
        """Consumes the global generators exactly as the reference's ``__getitem__`` does: ``np.random.randint`` for the
        start (first visit of a training item, every visit of a test item), segment picks for 'split-random', then
        ``random.random()`` for the flip, then the per-frame crop origins."""
        path = self.video_dirs[index]
        if self.spec.pick == 'all':
            files = [osp.join(path, f) for f in os.listdir(path)]        # directory order, as the reference
            flip = False
        else:
            length = len(os.listdir(path))
            skip = length // NUM_FRAMES if length < NUM_FRAMES * FRAME_GAP else FRAME_GAP
            if self.start[index] == -1 or self.split == "test":
                self.start[index] = int(np.random.randint(1, length - (NUM_FRAMES - 1) * skip))
            first = self.start[index]
            numbers = list(range(first, first + NUM_FRAMES * skip, skip))
            if self.family == 'miniUCF101' and self.sample == 'split-random':
                seg = length // 16
                bounds = [(k * seg, (k + 1) * seg if k < 15 else length) for k in range(16)]
                numbers = [int(np.random.randint(lo, hi)) + 1 for lo, hi in bounds]
            files = [osp.join(path, "frame{:06d}.jpg".format(n)) for n in numbers]
            flip = random.random() > 0.5
        crops = [self.transform.draw(0, 0) for _ in files]
        return ClipDraw(files, flip, crops)

    def read_u8(self, d: ClipDraw) -> np.ndarray:
        """-> (T, H, W, 3) uint8: decode, flip, resize / crop.  Thread-safe (no generator is touched)."""
        from PIL import Image
        frames = []
        for f, crop in zip(d.files, d.crops):
            with Image.open(f) as im:
                if d.flip:
                    im = im.transpose(Image.FLIP_LEFT_RIGHT)
                frames.append(self.transform.pixels(im, crop))
        return np.stack(frames, 0)

    def __getitem__(self, index: int):
        u8 = self.read_u8(self.draw(index))
        return self.transform.normalise(torch.from_numpy(u8)), self.labels[index]


# family -> (FolderSpec, how the one frame is chosen)
_STILL_SPECS = {
    'staticHMDB51': FolderSpec('csv-splits', 'hmdb51_splits.csv', 'jpegs_112', 'still'),
    'staticUCF101': FolderSpec('csv-splits', 'ucf101_splits1.csv', 'jpegs_112', 'still-part'),
    'staticUCF50': FolderSpec('csv-splits', 'ucf50_splits1_max.csv', 'jpegs_112', 'still-part'),
    'singleKinetics400': FolderSpec('csv-kinetics', '{split}.csv', '{split}', 'listed'),
    'singleSSv2': FolderSpec('json-ssv2', 'annot_{split}.json', 'frame', 'listed'),
}


class StillFrameVideos(FrameFolderVideos):
    """One frame per item.  The ``static*`` families draw a frame NUMBER with ``np.random.randint`` -- anywhere in the
    video (staticHMDB51, dataset.py:644), in the ``split_id``-th of ``split_num`` equal parts (staticUCF101 :730,
    staticUCF50 ``split_mode='mean'`` :823), or between the per-video cut points of the index file's ``split_index``
    column (staticUCF50 ``split_mode='feature'``, four parts, :824-830) -- then the flip, then ONE transform call, and
    return the frame stacked ``frames`` times, or as a (3, H, W) image when ``frames == 1`` (:626-633).  The ``single*``
    families (Kinetics400 / SSv2 frame sets) pick a listed file with ``random.randint`` and do not flip (:69-77, :938-947).
    A ``split_id`` outside ``split_num`` reads as 0 (:660, :746); the last frame of a video is never drawn, as in the
    reference (``randint``'s upper bound is the frame count)."""

    def __init__(self, family: str, path: str, split: str, transform: Optional[FrameTransform] = None, frames: int = NUM_FRAMES,
                 split_num: int = 1, split_id: int = 0, split_mode: str = 'mean'):
        if family not in _STILL_SPECS:
            raise ValueError("unknown still-frame family: %s" % family)
        self.family, self.spec, self.split, self.sample = family, _STILL_SPECS[family], split, 'random'
        self.transform = transform if transform is not None else FrameTransform((112, 112))
        self.root = path
        self.frames, self.split_num, self.split_mode = int(frames), int(split_num), split_mode
        self.split_id = 0 if split_id >= split_num else int(split_id)
        if family == 'staticUCF50' and split_mode not in ('mean', 'feature'):
            raise SystemExit("split_mode error!")                       # the reference exits on the first item (:831-833)
        self.split_lists: List[List[int]] = []
        names, label_strs, self.skipped = self._read_index(path, split)
        if family == 'staticUCF50':
            with open(osp.join(path, self.spec.index_file)) as fp:
                for row in csv.DictReader(fp):
                    if row["split"] == split:
                        self.split_lists.append(sorted(int(v) for v in row['split_index'].strip('][').split(', ')))
        self.video_dirs = names
        self.label_strs = label_strs
        self.class_strs = sorted(set(label_strs))
        self.class_2_idx = {s: i for i, s in enumerate(self.class_strs)}
        self.labels = [self.class_2_idx[s] for s in label_strs]
        self.targets = self.labels
        self.start = [-1] * len(self.video_dirs)                        # kept for shape; a still item redraws every visit

    def _expected_frames(self, path: str) -> int:
        return 8                                                        # dataset.py:20, 899 (both frame sets are 8 long)

    @property
    def image_items(self) -> bool:
        """Items are (3, H, W) images rather than (frames, 3, H, W) clips."""
        return self.spec.pick == 'listed' or self.frames == 1

    def _frame_range(self, index: int, length: int) -> Tuple[int, int]:
        if self.spec.pick == 'still':
            return 1, length
        if self.family == 'staticUCF50' and self.split_mode == 'feature':
            cuts = self.split_lists[index]
            if self.split_id == 0:
                return 1, cuts[0] + 1
            if self.split_id == 3:
                return cuts[2] + 1, length
            return cuts[self.split_id - 1] + 1, cuts[self.split_id] + 1
        part = length // self.split_num
        return part * self.split_id + 1, part * (self.split_id + 1)

    def draw(self, index: int) -> ClipDraw:
        path = self.video_dirs[index]
        listing = os.listdir(path)
        if self.spec.pick == 'listed':
            files = [osp.join(path, listing[random.randint(0, len(listing) - 1)])]
            flip = False
        else:
            lo, hi = self._frame_range(index, len(listing))
            number = int(np.random.randint(lo, hi))
            self.start[index] = number
            files = [osp.join(path, "frame{:06d}.jpg".format(number))]
            flip = random.random() > 0.5
        return ClipDraw(files, flip, [self.transform.draw(0, 0)])

    def __getitem__(self, index: int):
        image = self.transform.normalise(torch.from_numpy(self.read_u8(self.draw(index))))[0]
        if self.image_items:
            return image, self.labels[index]
        return torch.stack([image] * self.frames, 0), self.labels[index]


def staticHMDB51(path, split, transform=None, frames=NUM_FRAMES):
    return StillFrameVideos('staticHMDB51', path, split, transform, frames)


def staticUCF101(path, split, transform=None, frames=NUM_FRAMES, split_num=1, split_id=0):
    return StillFrameVideos('staticUCF101', path, split, transform, frames, split_num, split_id)


def staticUCF50(path, split, transform=None, frames=NUM_FRAMES, split_num=1, split_id=0, split_mode='mean'):
    return StillFrameVideos('staticUCF50', path, split, transform, frames, split_num, split_id, split_mode)


def singleKinetics400(path, split, transform=None):
    return StillFrameVideos('singleKinetics400', path, split, transform)


def singleSSv2(path, split, transform=None):
    return StillFrameVideos('singleSSv2', path, split, transform)


def UCF101(path, split, transform=None):
    return FrameFolderVideos('UCF101', path, split, transform)


def HMDB51(path, split, transform=None):
    return FrameFolderVideos('HMDB51', path, split, transform)


def miniUCF101(path, split, transform=None, sample='random'):
    return FrameFolderVideos('miniUCF101', path, split, transform, sample)


def miniHMDB51(path, split, transform=None):
    return FrameFolderVideos('miniHMDB51', path, split, transform)


def Kinetics400(path, split, transform=None):
    return FrameFolderVideos('Kinetics400', path, split, transform)


def SSv2(path, split, transform=None):
    return FrameFolderVideos('SSv2', path, split, transform)


# name -> (family, sub-directory of data_path, num_classes, fixed im_size or None)   utils.py:132-236
_DATASETS = {
    'Kinetics400': ('Kinetics400', 'Kinetics', 400, (64, 64)),
    'Kinetics400_long': ('Kinetics400', 'kinetics_112x112x16', 400, (112, 112)),
    'UCF101': ('UCF101', 'UCF101', 101, None),
    'HMDB51': ('HMDB51', 'HMDB51', 51, None),
    'miniUCF101': ('miniUCF101', 'UCF101', 50, None),
}                                                   # (the reference has a video ``SSv2`` class but no get_dataset branch for it)


# still-image names -> (family, sub-directory, num_classes, fixed im_size or None, frames, passes the split arguments)   utils.py:237-454
_STILL_DATASETS = {
    'staticHMDB51': ('staticHMDB51', 'HMDB51', 51, None, NUM_FRAMES, False),
    'staticUCF101': ('staticUCF101', 'UCF101', 101, None, NUM_FRAMES, False),
    'staticUCF50': ('staticUCF50', 'UCF101', 50, None, NUM_FRAMES, False),
    'singleHMDB51': ('staticHMDB51', 'HMDB51', 51, None, 1, False),
    'singleUCF50': ('staticUCF50', 'UCF101', 50, None, 1, True),
    'singleUCF101': ('staticUCF101', 'UCF101', 101, None, 1, True),
    'singleKinetics400': ('singleKinetics400', 'Kinetics', 400, (64, 64), 1, False),
    'singleSSv2': ('singleSSv2', 'SSv2', 174, (64, 64), 1, False),
}


def get_dataset(dataset: str, data_path: str, num_workers: int = 0, img_size=(112, 112), split_num: int = 1, split_id: int = 0,
                split_mode: str = 'mean'):
    """The video and still-frame branches of the reference's ``get_dataset`` (utils.py:21, 132-454, 507-508): same 9-tuple
    ``(channel, im_size, num_classes, class_names, mean, std, dst_train, dst_test, testloader)``.  Unknown names end the
    process as the reference does (utils.py:505).  The split arguments reach only ``singleUCF50`` / ``singleUCF101``
    (utils.py:380-381, 411-412); ``singleHMDB51`` resizes + crops only for 64x64 targets (utils.py:345), the others for any
    size that is not the stored 112x112."""
    if dataset in _STILL_DATASETS:
        family, sub, num_classes, fixed, frames, splits = _STILL_DATASETS[dataset]
        im_size = tuple(fixed) if fixed is not None else tuple(img_size)
        path = data_path + "/" + sub
        assert os.path.exists(path), path
        listed = _STILL_SPECS[family].pick == 'listed'
        plain = listed or (dataset == 'singleHMDB51' and im_size != (64, 64))
        transform = FrameTransform(im_size, stored=im_size if plain else (112, 112))
        kw = dict(split_num=split_num, split_id=split_id) if splits else {}
        if splits and family == 'staticUCF50':
            kw['split_mode'] = split_mode
        dst_train = StillFrameVideos(family, path, "train", transform, frames, **kw)
        dst_test = StillFrameVideos(family, path, "val" if listed else "test", transform, frames, **kw)
        testloader = tdata.DataLoader(dst_test, batch_size=64, shuffle=False, num_workers=num_workers)
        return 3, im_size, num_classes, None, list(IMAGENET_MEAN), list(IMAGENET_STD), dst_train, dst_test, testloader
    if dataset not in _DATASETS:
        raise SystemExit('unknown dataset: %s' % dataset)
    family, sub, num_classes, fixed = _DATASETS[dataset]
    im_size = tuple(fixed) if fixed is not None else tuple(img_size)
    path = data_path + "/" + sub
    assert os.path.exists(path), path
    listed = SPECS[family].pick == 'all'            # pre-resized frame sets: no Resize / RandomCrop branch
    transform = FrameTransform(im_size, stored=im_size if listed else (112, 112))
    test_split = "val" if listed else "test"
    dst_train = FrameFolderVideos(family, path, "train", transform)
    dst_test = FrameFolderVideos(family, path, test_split, transform)
    testloader = tdata.DataLoader(dst_test, batch_size=64, shuffle=False, num_workers=num_workers)
    return 3, im_size, num_classes, None, list(IMAGENET_MEAN), list(IMAGENET_STD), dst_train, dst_test, testloader


# ------------------------------------------------------------------------------------------------------------------------
# HBM-resident preload
# ------------------------------------------------------------------------------------------------------------------------
def frames_normalize(u8: torch.Tensor, out: torch.Tensor, mean: Sequence[float], std: Sequence[float]) -> torch.Tensor:
    """(n, H, W, 3) uint8 on the device -> ``out`` (n, 3, H, W) fp32 by ``vd_frames_normalize`` on the current stream."""
    import ctypes
    from . import hip
    n, h, w, c = u8.shape
    assert c == 3 and u8.dtype == torch.uint8 and u8.is_contiguous() and u8.is_cuda
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == u8.numel() and out.device == u8.device
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    with torch.cuda.device(u8.device):
        hip.run("vd_frames_normalize", hip.ptr(u8), hip.ptr(out), n, int(h), int(w), m, s, hip.stream_ptr(u8.device))
    return out


def preload(dataset: FrameFolderVideos, device, indices: Optional[Sequence[int]] = None, workers: int = 8, chunk: int = 64):
    """Every item of ``dataset`` (or of ``indices``, in that order) decoded once and left in HBM.

    -> ``(clips (N, T, 3, H, W) fp32 on ``device`` -- (N, 3, H, W) for the image items of ``StillFrameVideos`` --, labels
    (N,) int64 on the host)``; the same values
    ``torch.stack([dataset[i][0] for i in indices])`` produces (the draws happen here, in index order; only the file reads
    run on the ``workers`` threads), with 1/4 of the bytes crossing PCIe and the normalisation done by the device.
    The copy of chunk k+1 overlaps the decode of chunk k+2 and the normalisation of chunk k (pinned double buffer, one
    copy stream)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dataset.preload: the preload targets HBM; use dataset[i] for host tensors")
    idx = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    labels = torch.tensor([dataset.labels[i] for i in idx], dtype=torch.int64)
    if not idx:
        return torch.empty((0, 0, 3, 0, 0), device=device), labels
    draws = [dataset.draw(i) for i in idx]                     # generator order = item order
    tf = dataset.transform
    first = dataset.read_u8(draws[0])
    t, h, w, _ = first.shape
    clips = torch.empty((len(idx), t, 3, h, w), dtype=torch.float32, device=device)
    copy_stream = torch.cuda.Stream(device=device)
    main = torch.cuda.current_stream(device)
    stage = [torch.empty((chunk, t, h, w, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
    dev_u8 = [torch.empty((chunk, t, h, w, 3), dtype=torch.uint8, device=device) for _ in range(2)]
    landed = [torch.cuda.Event() for _ in range(2)]          # H2D of the buffer finished
    drained = [torch.cuda.Event() for _ in range(2)]         # normalise kernel has read the device buffer
    used = [False, False]

    def decode_into(buf, k, item):
        got = first if item == 0 else dataset.read_u8(draws[item])
        if got.shape != (t, h, w, 3):
            raise ValueError("clip %s has shape %s, the first one %s" % (draws[item].files[0], got.shape, (t, h, w, 3)))
        buf[k] = torch.from_numpy(got)

    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
        for ci, lo in enumerate(range(0, len(idx), chunk)):
            b = ci & 1
            n = min(chunk, len(idx) - lo)
            if used[b]:
                landed[b].synchronize()                        # the pinned buffer may be overwritten
            list(pool.map(lambda k: decode_into(stage[b], k, lo + k), range(n)))
            with torch.cuda.stream(copy_stream):
                if used[b]:
                    copy_stream.wait_event(drained[b])
                dev_u8[b][:n].copy_(stage[b][:n], non_blocking=True)
                landed[b].record(copy_stream)
            main.wait_event(landed[b])
            frames_normalize(dev_u8[b][:n].view(n * t, h, w, 3), clips[lo:lo + n].view(n * t, 3, h, w), tf.mean.tolist(), tf.std.tolist())
            drained[b].record(main)
            used[b] = True
    main.synchronize()
    if isinstance(dataset, StillFrameVideos):                   # one decoded frame per item: an image, or that frame repeated on the device
        clips = clips[:, 0] if dataset.image_items else clips.expand(-1, dataset.frames, -1, -1, -1).contiguous()
    return clips, labels


def indices_class(labels: Sequence[int], num_classes: int) -> List[List[int]]:
    """``indices_class[c]`` = item numbers of class c in dataset order (distill_baseline.py:76-81)."""
    out: List[List[int]] = [[] for _ in range(num_classes)]
    for i, lab in enumerate(labels):
        out[int(lab)].append(i)
    return out


class DeviceBatches:
    """Mini-batches of an HBM-resident tensor set: what ``DataLoader(TensorDataset(clips, labels), batch_size, shuffle)``
    yields (buffer.py:62, utils.py:861), without a per-item host loop — one ``index_select`` per batch on the device.
    The shuffle consumes the global torch generator exactly as the DataLoader does (one int64 for the iterator's base
    seed, one for the sampler's seed, then ``randperm`` from a generator seeded with the latter), so a seeded run sees the
    same batches either way; the last batch is short."""

    def __init__(self, clips: torch.Tensor, labels: torch.Tensor, batch_size: int, shuffle: bool = False, generator=None):
        assert clips.shape[0] == labels.shape[0]
        self.clips, self.labels = clips, labels.to(clips.device)
        self.batch_size, self.shuffle, self.generator = int(batch_size), bool(shuffle), generator

    def __len__(self) -> int:
        return (self.clips.shape[0] + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = self.clips.shape[0]
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)          # the iterator's base seed
        if self.shuffle:
            if self.generator is None:
                gen = torch.Generator()
                gen.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
            else:
                gen = self.generator
            order = torch.randperm(n, generator=gen)
        else:
            order = torch.arange(n)
        order = order.to(self.clips.device)
        for lo in range(0, n, self.batch_size):
            idx = order[lo:lo + self.batch_size]
            yield self.clips.index_select(0, idx), self.labels.index_select(0, idx)
        if self.shuffle and self.generator is not None:
            torch.randperm(n, generator=self.generator)      # RandomSampler ends an epoch with a second (unused) permutation


# ------------------------------------------------------------------------------------------------------------------------
# HBM-resident whole videos, clips drawn per read on the device
# ------------------------------------------------------------------------------------------------------------------------
def sample_clips(frames: torch.Tensor, frame_row, flip, crop_yx, frames_per_clip: int, out_hw: Tuple[int, int],
                 mean: Sequence[float], std: Sequence[float]):
    """``vd_clips_sample`` on the current stream: ``frames`` (F, Hs, Ws, 3) uint8 on the device, HOST tables ``frame_row``
    (nclips * T) / ``flip`` (nclips) / ``crop_yx`` (nclips * T, 2) or None -> a fresh (nclips, T, 3, H, W) fp32 tensor.

    The tables are validated here, on the host (a row outside the store or a crop past the edge raises ``ValueError``: it
    never reaches the device), packed into ONE pinned buffer and uploaded with one asynchronous copy; nothing synchronises."""
    out, _ = _sample_clips(frames, frame_row, flip, crop_yx, frames_per_clip, out_hw, mean, std, None)
    return out


def check_clip_tables(store_frames: int, src_hw, out_hw, frame_row, flip, crop_yx, frames_per_clip: int):
    """Host-side bounds check of the tables of one ``vd_clips_sample`` call -> (rows int64, flips uint8, crops int32 or None)
    as contiguous numpy arrays.  ``ValueError`` for anything the kernel must not be handed."""
    rows = np.ascontiguousarray(np.asarray(frame_row, dtype=np.int64).reshape(-1))
    flips = np.ascontiguousarray(np.asarray(flip).astype(np.uint8).reshape(-1))
    t = int(frames_per_clip)
    (hs, ws), (oh, ow) = (int(v) for v in src_hw), (int(v) for v in out_hw)
    if t <= 0 or rows.size != flips.size * t:
        raise ValueError("clip tables: %d rows for %d clips of %d frames" % (rows.size, flips.size, t))
    if oh > hs or ow > ws or oh < 0 or ow < 0:
        raise ValueError("clip tables: output %s is larger than the stored frame %s" % ((oh, ow), (hs, ws)))
    if rows.size and (rows.min() < 0 or rows.max() >= store_frames):
        bad = int(rows[(rows < 0) | (rows >= store_frames)][0])
        raise ValueError("clip tables: frame row %d is outside the store (%d frames)" % (bad, store_frames))
    if crop_yx is None:
        if (oh, ow) != (hs, ws):
            raise ValueError("clip tables: output %s differs from the stored frame %s and there is no crop" % ((oh, ow), (hs, ws)))
        return rows, flips, None
    crops = np.ascontiguousarray(np.asarray(crop_yx, dtype=np.int64).reshape(-1, 2))
    if crops.shape[0] != rows.size:
        raise ValueError("clip tables: %d crop origins for %d frames" % (crops.shape[0], rows.size))
    if crops.size and (crops.min() < 0 or crops[:, 0].max() > hs - oh or crops[:, 1].max() > ws - ow):
        k = int(np.nonzero((crops[:, 0] < 0) | (crops[:, 1] < 0) | (crops[:, 0] > hs - oh) | (crops[:, 1] > ws - ow))[0][0])
        raise ValueError("clip tables: crop origin %s + %s runs past the edge of the stored frame %s"
                         % (tuple(int(v) for v in crops[k]), (oh, ow), (hs, ws)))
    return rows, flips, crops.astype(np.int32)


def _sample_clips(frames, frame_row, flip, crop_yx, frames_per_clip, out_hw, mean, std, extra):
    """``sample_clips`` + ``extra``: an optional int64 host array that rides in the same upload (the batch's labels);
    -> (clips, its device copy or None)."""
    import ctypes
    from . import hip
    assert frames.dim() == 4 and frames.shape[3] == 3 and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.is_cuda
    store_frames, hs, ws = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    oh, ow = int(out_hw[0]), int(out_hw[1])
    t = int(frames_per_clip)
    rows, flips, crops = check_clip_tables(store_frames, (hs, ws), (oh, ow), frame_row, flip, crop_yx, t)
    b, nf = flips.size, rows.size
    out = torch.empty((b, t, 3, oh, ow), dtype=torch.float32, device=frames.device)
    ne = 0 if extra is None else int(np.asarray(extra).size)
    if b == 0:
        return out, (None if extra is None else torch.empty((0,), dtype=torch.int64, device=frames.device))
    # one pinned buffer, 8-byte aligned sections: rows (int64) | crops (int32 pairs) | extra (int64) | flips (uint8).  A fresh
    # pinned block per call: the caching host allocator hands it out again only after the copy below has finished.
    o_crop = 8 * nf
    o_extra = o_crop + (8 * nf if crops is not None else 0)
    o_flip = o_extra + 8 * ne
    host = torch.empty((o_flip + b,), dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    hv[:o_crop].view(np.int64)[:] = rows
    if crops is not None:
        hv[o_crop:o_extra].view(np.int32)[:] = crops.reshape(-1)
    if ne:
        hv[o_extra:o_flip].view(np.int64)[:] = np.asarray(extra, dtype=np.int64).reshape(-1)
    hv[o_flip:] = flips
    dev = host.to(frames.device, non_blocking=True)
    base = dev.data_ptr()
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    with torch.cuda.device(frames.device):
        hip.run("vd_clips_sample", hip.ptr(frames), store_frames, hs, ws, base, (base + o_crop if crops is not None else 0),
                base + o_flip, b, t, oh, ow, hip.ptr(out), m, s, hip.stream_ptr(frames.device))
    return out, (dev[o_extra:o_flip].view(torch.int64) if extra is not None else None)


@dataclass
class ResidentDraw:
    """Everything random about one read of a resident video: frame NUMBERS (1-based, as in the file names), flip, crops."""
    index: int
    numbers: List[int]
    flip: bool
    crops: List[Optional[Tuple[int, int]]]


class ResidentVideos:
    """Every frame of every video of a 'window' dataset (UCF101, HMDB51, miniUCF101 -- 'split-random' included --, miniHMDB51),
    decoded ONCE and kept in HBM as ``frames (F, Hs, Ws, 3) uint8``: RGB, resized when the transform resizes, neither flipped
    nor cropped (PIL's flip and its bilinear resize commute byte for byte, so the flip of a read is a mirrored read of the
    stored frame).  ``frame_offset (N+1)``, ``length (N)`` and ``labels`` stay on the host.  What a read draws -- start frame
    per visit of a test item, segment picks, flip, crop origins -- is drawn per read by ``draw``, in the generator order of
    ``FrameFolderVideos.draw``, and turned into a normalised batch by ``vd_clips_sample`` (``batch``): the clips the
    reference's datasets produce, without a JPEG decode per read.

    The constructor only lists directories (lengths, offsets, ``nbytes``); ``load`` decodes and uploads;
    ``from_dataset`` does both."""

    def __init__(self, dataset: FrameFolderVideos, indices: Optional[Sequence[int]] = None):
        if isinstance(dataset, StillFrameVideos) or not isinstance(dataset, FrameFolderVideos):
            raise ValueError("ResidentVideos: a still-frame dataset picks one frame per item and has no clip to draw per read; "
                             "use dataset.preload")
        if dataset.spec.pick != 'window':
            raise ValueError("ResidentVideos: the %s family reads every listed frame of a video (no per-read frame choice); "
                             "use dataset.preload" % dataset.family)
        self.dataset = dataset
        self.indices = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
        self.slot = {i: k for k, i in enumerate(self.indices)}
        self.length = [len(os.listdir(dataset.video_dirs[i])) for i in self.indices]
        self.frame_offset = np.concatenate([[0], np.cumsum(self.length, dtype=np.int64)]).astype(np.int64)
        self.labels = torch.tensor([dataset.labels[i] for i in self.indices], dtype=torch.int64)
        tf = dataset.transform
        self.out_hw = tuple(tf.im_size) if tf.resize is not None else None      # (None: the stored size, known below)
        self._frame_hw = tuple(tf.resize) if tf.resize is not None else None
        self.frames: Optional[torch.Tensor] = None
        self.build_seconds = None

    # -- sizes, from the listing alone ---------------------------------------------------------------------------------------
    @property
    def num_frames(self) -> int:
        return int(self.frame_offset[-1])

    @property
    def frame_hw(self) -> Tuple[int, int]:
        """Stored frame size: the transform's resize target, or the size in the header of the first frame file (no decode)."""
        if self._frame_hw is None:
            if not self.indices:
                raise ValueError("ResidentVideos: an empty store has no frame size")
            from PIL import Image
            with Image.open(self._file(0, 1)) as im:
                self._frame_hw = (im.height, im.width)
        return self._frame_hw

    @property
    def nbytes(self) -> int:
        """Bytes of ``frames``: F x Hs x Ws x 3."""
        if not self.num_frames:
            return 0
        h, w = self.frame_hw
        return self.num_frames * h * w * 3

    def _file(self, slot: int, number: int) -> str:
        return osp.join(self.dataset.video_dirs[self.indices[slot]], "frame{:06d}.jpg".format(number))

    # -- build ---------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_dataset(cls, dataset: FrameFolderVideos, device, indices: Optional[Sequence[int]] = None, workers: int = 8,
                     max_bytes: Optional[int] = None) -> "ResidentVideos":
        return cls(dataset, indices).load(device, workers=workers, max_bytes=max_bytes)

    def load(self, device, workers: int = 8, max_bytes: Optional[int] = None, chunk: int = 2048) -> "ResidentVideos":
        """Decode every frame on ``workers`` host threads (16 at most) and copy it into HBM through a pinned double buffer on
        a copy stream.  Refuses (``ValueError``, before anything is decoded) a store larger than ``max_bytes`` -- by default
        half of the device's free memory."""
        import time
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ResidentVideos: the store lives in HBM; use dataset[i] for host tensors")
        need = self.nbytes
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(device)[0] // 2
        if need > int(max_bytes):
            raise ValueError("ResidentVideos: %d videos / %d frames need %d bytes of HBM, more than max_bytes = %d; build the store "
                             "over fewer videos (indices=) or raise max_bytes" % (len(self.indices), self.num_frames, need, int(max_bytes)))
        t0 = time.time()
        nf = self.num_frames
        if nf == 0:
            self.frames = torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device)
            self.build_seconds = 0.0
            return self
        h, w = self.frame_hw
        if self.out_hw is None:
            self.out_hw = (h, w)
        tf = self.dataset.transform
        frames = torch.empty((nf, h, w, 3), dtype=torch.uint8, device=device)
        where = [(k, n) for k in range(len(self.indices)) for n in range(1, self.length[k] + 1)]      # store row -> (slot, number)
        chunk = max(1, min(int(chunk), nf))
        stage = [torch.empty((chunk, h, w, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        landed = [torch.cuda.Event() for _ in range(2)]
        used = [False, False]
        copy_stream = torch.cuda.Stream(device=device)
        from PIL import Image

        def decode_into(buf, k, row):
            slot, number = where[row]
            with Image.open(self._file(slot, number)) as im:
                got = tf.stored_pixels(im)
            if got.shape != (h, w, 3):
                raise ValueError("ResidentVideos: %s is %s, the first frame %s (videos of mixed frame sizes cannot share a store)"
                                 % (self._file(slot, number), got.shape[:2], (h, w)))
            buf[k] = got

        views = [s.numpy() for s in stage]                     # (numpy views of the pinned buffers: PIL's arrays are read-only)
        with ThreadPoolExecutor(max_workers=max(1, min(int(workers), 16))) as pool:
            for ci, lo in enumerate(range(0, nf, chunk)):
                b = ci & 1
                n = min(chunk, nf - lo)
                if used[b]:
                    landed[b].synchronize()                    # the pinned buffer may be overwritten
                list(pool.map(lambda k: decode_into(views[b], k, lo + k), range(n)))
                with torch.cuda.stream(copy_stream):
                    frames[lo:lo + n].copy_(stage[b][:n], non_blocking=True)
                    landed[b].record(copy_stream)
                used[b] = True
        copy_stream.synchronize()
        self.frames = frames
        self.build_seconds = time.time() - t0
        return self

    def __len__(self) -> int:
        return len(self.indices)

    # -- one read: the draws, then the tables --------------------------------------------------------------------------------
    def draw(self, index: int) -> ResidentDraw:
        """The draws of ``dataset[index]``, consumed from the global generators exactly as ``FrameFolderVideos.draw`` consumes
        them (``np.random.randint`` for the start -- every visit of a test item, the first visit of any other --, the segment
        picks of 'split-random', ``random.random()`` for the flip, ``torch.randint`` per frame when the transform crops), from
        the cached lengths (no ``listdir``).  The start is the dataset's own ``start[index]``: host reads and resident reads of
        one dataset see the same cached start."""
        ds = self.dataset
        index = int(index)
        if index not in self.slot:
            raise ValueError("ResidentVideos: item %d is not in the store" % index)
        length = self.length[self.slot[index]]
        skip = length // NUM_FRAMES if length < NUM_FRAMES * FRAME_GAP else FRAME_GAP
        if ds.start[index] == -1 or ds.split == "test":
            ds.start[index] = int(np.random.randint(1, length - (NUM_FRAMES - 1) * skip))
        first = ds.start[index]
        numbers = list(range(first, first + NUM_FRAMES * skip, skip))
        if ds.family == 'miniUCF101' and ds.sample == 'split-random':
            seg = length // 16
            bounds = [(k * seg, (k + 1) * seg if k < 15 else length) for k in range(16)]
            numbers = [int(np.random.randint(lo, hi)) + 1 for lo, hi in bounds]
        flip = random.random() > 0.5
        crops = [ds.transform.draw(0, 0) for _ in numbers]
        return ResidentDraw(index, numbers, flip, crops)

    def tables(self, draws: Sequence[ResidentDraw]):
        """Host tables of a batch of draws -> ``(frame_row (b*T) int64, flip (b) uint8, crop_yx (b*T, 2) int32 or None)``,
        validated against ``frame_offset`` / ``length`` and the crop bounds (``ValueError`` otherwise).  Needs no device."""
        t = NUM_FRAMES
        rows = np.empty((len(draws), t), dtype=np.int64)
        flips = np.empty((len(draws),), dtype=np.uint8)
        cropped = self.dataset.transform.resize is not None
        crops = np.empty((len(draws), t, 2), dtype=np.int32) if cropped else None
        for b, d in enumerate(draws):
            if d.index not in self.slot:
                raise ValueError("ResidentVideos: item %d is not in the store" % d.index)
            slot = self.slot[d.index]
            if len(d.numbers) != t:
                raise ValueError("ResidentVideos: a draw of %d frames, clips have %d" % (len(d.numbers), t))
            for n in d.numbers:
                if not 1 <= int(n) <= self.length[slot]:
                    raise ValueError("ResidentVideos: frame %d of %s is out of range (the video has %d frames)"
                                     % (int(n), self.dataset.video_dirs[d.index], self.length[slot]))
            rows[b] = self.frame_offset[slot] + np.asarray(d.numbers, dtype=np.int64) - 1
            flips[b] = 1 if d.flip else 0
            if cropped:
                if len(d.crops) != t or any(c is None for c in d.crops):
                    raise ValueError("ResidentVideos: the transform crops, a draw without %d crop origins" % t)
                crops[b] = np.asarray(d.crops, dtype=np.int32)
        out_hw = self.out_hw if self.out_hw is not None else self.frame_hw
        return check_clip_tables(self.num_frames, self.frame_hw if self.num_frames else (0, 0), out_hw, rows.reshape(-1), flips,
                                 None if crops is None else crops.reshape(-1, 2), t)

    def batch(self, draws: Sequence[ResidentDraw]):
        """-> ``(clips (b, T, 3, H, W) fp32, labels (b,) int64)`` on the store's device, fresh tensors; one table upload and
        one ``vd_clips_sample`` launch on the current stream, no synchronisation."""
        if self.frames is None:
            raise RuntimeError("ResidentVideos: the store has not been loaded (from_dataset / load)")
        rows, flips, crops = self.tables(draws)
        tf = self.dataset.transform
        labels = np.asarray([self.dataset.labels[d.index] for d in draws], dtype=np.int64)
        return _sample_clips(self.frames, rows, flips, crops, NUM_FRAMES, self.out_hw, tf.mean.tolist(), tf.std.tolist(), labels)


class ResidentClipLoader:
    """Drop-in for ``DataLoader(dataset, batch_size, shuffle, num_workers=0)`` over a ``ResidentVideos`` store: iterating yields
    ``(clips (b, T, 3, H, W) fp32, labels (b,) int64)`` on the store's device, the last batch short.  The global generators are
    consumed exactly as the DataLoader iterating ``dataset[i]`` consumes them -- the iterator's base seed, the sampler's seed and
    ``randperm`` (as ``DeviceBatches``), then the draws of every item in batch order -- so a seeded run sees the same clips either
    way and leaves the generators in the same state."""

    def __init__(self, store: ResidentVideos, batch_size: int = 64, shuffle: bool = False, generator=None):
        self.store, self.dataset = store, store.dataset
        self.batch_size, self.shuffle, self.generator = int(batch_size), bool(shuffle), generator

    def __len__(self) -> int:
        return (len(self.store) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.store)
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)          # the iterator's base seed
        if self.shuffle:
            if self.generator is None:
                gen = torch.Generator()
                gen.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
            else:
                gen = self.generator
            order = torch.randperm(n, generator=gen).tolist()
        else:
            order = list(range(n))
        for lo in range(0, n, self.batch_size):
            yield self.store.batch([self.store.draw(self.store.indices[k]) for k in order[lo:lo + self.batch_size]])
        if self.shuffle and self.generator is not None:
            torch.randperm(n, generator=self.generator)      # RandomSampler ends an epoch with a second (unused) permutation


def resident_loader(dataset: FrameFolderVideos, device, batch_size: int = 64, shuffle: bool = False, workers: int = 8,
                    max_bytes: Optional[int] = None) -> ResidentClipLoader:
    """``ResidentVideos.from_dataset`` + ``ResidentClipLoader`` in one call."""
    return ResidentClipLoader(ResidentVideos.from_dataset(dataset, device, workers=workers, max_bytes=max_bytes), batch_size, shuffle)
