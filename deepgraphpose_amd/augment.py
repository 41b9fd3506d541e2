"""Host-side augmentation of the labeled frames of a DGP batch.

Counterpart of `build_aug` / `data_aug` (DGP/models/fitdgp_util.py:412-451): the reference chains seven imgaug
augmenters, each behind `Sometimes(apply_prob)`, over the VISIBLE frames of a batch and moves the labels with the
pixels.  imgaug is a third-party host library the reference only calls; when it is importable `build_aug` returns the
reference's own pipeline object, otherwise the numpy / scipy pipeline below, which draws the same parameters from the
same distributions (own RNG stream: imgaug's bit stream is not reproducible without imgaug):

  Fliplr(0.5) | Affine(rotate=(-10, 10)) | MotionBlur(k=3, angle=(-90, 90)) | CoarseDropout((0, 0.02), size_percent=(0.01, 0.05))
  | ElasticTransformation(sigma=5, alpha=(0, 10)) | AdditiveGaussianNoise(scale=(0, 0.01*255), per_channel=0.5)
  | Sometimes(0.4, CropAndPad(percent=(-0.3, 0.1), keep_size=True))

Keypoints are (x, y) pixel coordinates, NaN = unlabeled (NaNs stay NaN).  Both pipelines are called as
`pipeline(images=uint8 [n,H,W,3], keypoints=[[(x, y), ...], ...]) -> (images, keypoints)`.

Every draw of the numpy pipeline is independent of the pixels and its array shapes depend on (H, W) alone, so each augmenter is split
in two: `NumpyAugPipeline.draw_<stage>(H, W)` draws the stage's parameters (the only code that touches the RNG) and the module's
`apply_<stage>(img, kp, params)` applies them.  A frame's augmentation is a PLAN, the list of (stage, params) of the stages whose
`Sometimes` coin came up, drawn first and applied afterwards: on the host (`apply_host`) or on the device
(engine.augment_frames, csrc/dgp_augment.hip), the keypoints on the host either way (`keypoints_of`).
"""
from __future__ import annotations

import numpy as np

STAGES = ("fliplr", "rotate", "motion_blur", "coarse_dropout", "elastic", "gaussian_noise", "crop_and_pad")
NOISE_SOURCES = ("field", "key")
ELASTIC_STEP = 4                # the elastic field is drawn on every 4th pixel


# ---- the pixel half and the keypoint half of each stage: pure functions of the drawn parameters --------------------------------------
# image uint8 [H, W, C]; keypoints float64 [nj, 2] as (x, y); H, W: the frame's size (no stage changes it)

def _kp_same(kp, params, H, W):
    return kp


def _px_fliplr(img, params):
    return img[:, ::-1] if params["flip"] else img


def _kp_fliplr(kp, params, H, W):
    if not params["flip"]:
        return kp
    kp = kp.copy()
    kp[:, 0] = W - kp[:, 0]
    return kp


def rotate_coefficients(deg, H, W):
    """-> (Pillow's six AFFINE coefficients, R, c): output = R (input - c) + c in (x, y), a rotation by `deg` about the image centre"""
    t = np.deg2rad(deg)
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])                      # rotation about the image centre, (x, y)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])   # output = R (input - c) + c in (x, y)
    Ri = R.T                                                          # inverse map for the resampler: in = Ri (out - c) + c
    off = c - Ri @ c
    # PIL samples the input at a (xo + 0.5) + b (yo + 0.5) + c0 - 0.5 (pixel-centre convention); fold the halves into c0 / f0 so
    # that pixel INDICES map as in = Ri out + off (bilinear, zeros outside -- imgaug's Affine defaults: order 1, cval 0)
    a_, b_, d_, e_ = Ri[0, 0], Ri[0, 1], Ri[1, 0], Ri[1, 1]
    c0 = off[0] + 0.5 - 0.5 * (a_ + b_)
    f0 = off[1] + 0.5 - 0.5 * (d_ + e_)
    return (float(a_), float(b_), float(c0), float(d_), float(e_), float(f0)), R, c


def _px_rotate(img, params):
    from PIL import Image
    H, W = img.shape[:2]
    return np.asarray(Image.fromarray(img).transform((W, H), Image.AFFINE, params["coef"], resample=Image.BILINEAR))


def _kp_rotate(kp, params, H, W):
    _, R, c = rotate_coefficients(params["deg"], H, W)
    return (kp - c) @ R.T + c


def motion_blur_kernel(deg):
    """MotionBlur(k=3)'s 3 x 3 fp32 kernel: a 3-tap line through the centre at `deg` degrees (bilinear weights), normalised"""
    ang = np.deg2rad(deg)
    k = np.zeros((3, 3), dtype=np.float32)
    k[1, 1] = 1.0
    dx, dy = np.cos(ang), np.sin(ang)
    for s in (-1, 1):
        x, y = 1 + s * dx, 1 + s * dy
        x0, y0 = int(np.floor(x)), int(np.floor(y))
        for yy, wy in ((y0, 1 - (y - y0)), (y0 + 1, y - y0)):
            for xx, wx in ((x0, 1 - (x - x0)), (x0 + 1, x - x0)):
                if 0 <= yy < 3 and 0 <= xx < 3:
                    k[yy, xx] += wy * wx
    k /= k.sum()
    return k


def _px_motion_blur(img, params):
    # 3 x 3 convolution (correlation with the flipped kernel), borders repeat the edge pixel (scipy's "reflect" at pad 1), all
    # channels at once: a sum of the shifted images with non-zero weight
    k = params["kernel"]
    H, W = img.shape[:2]
    pad = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge").astype(np.float32)
    out = np.zeros(img.shape, dtype=np.float32)
    for yy in range(3):
        for xx in range(3):
            wgt = k[2 - yy, 2 - xx]
            if wgt != 0.0:
                out += np.float32(wgt) * pad[yy:yy + H, xx:xx + W]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def _px_coarse_dropout(img, params):
    drop = params["mask"]
    H, W = img.shape[:2]
    h, w = drop.shape
    rows = np.minimum((np.arange(H) * h) // H, h - 1)
    cols = np.minimum((np.arange(W) * w) // W, w - 1)
    mask = drop[rows][:, cols]                                        # nearest-neighbour upsampling of the coarse mask
    out = img.copy()
    out[mask] = 0
    return out


def elastic_shift(params, H, W):
    """The full-resolution displacement of the elastic stage, torch fp32 [2, H, W] (dx, dy): the coarse field brought to every pixel
    bilinearly (align_corners: node (i, j) sits on pixel (4 i, 4 j))"""
    import torch
    import torch.nn.functional as F
    S = ELASTIC_STEP
    field = params["field"]
    hc, wc = field.shape[1:]
    d = torch.from_numpy(np.ascontiguousarray(field, dtype=np.float32))[None]                # [1, 2, hc, wc]
    return F.interpolate(d, size=(S * (hc - 1) + 1, S * (wc - 1) + 1), mode="bilinear", align_corners=True)[0, :, :H, :W]


def _elastic_pixels(img, d):
    import torch
    import torch.nn.functional as F
    H, W = img.shape[:2]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gx = (xx + d[0]) * (2.0 / max(W - 1, 1)) - 1.0
    gy = (yy + d[1]) * (2.0 / max(H - 1, 1)) - 1.0
    src = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)[None].float()
    out = F.grid_sample(src, torch.stack([gx, gy], -1)[None], mode="bilinear", padding_mode="zeros", align_corners=True)
    return out[0].permute(1, 2, 0).round_().clamp_(0, 255).to(torch.uint8).numpy()


def _elastic_keypoints(kp, d, H, W):
    kp2 = kp.copy()
    dn = d.numpy()
    for j in range(kp.shape[0]):                                      # out[p] = in[p + d(p)]  =>  a point moves by about -d
        x, y = kp[j]
        if np.isfinite(x) and np.isfinite(y):
            xi, yi = int(np.clip(round(x), 0, W - 1)), int(np.clip(round(y), 0, H - 1))
            kp2[j, 0] = x - dn[0, yi, xi]
            kp2[j, 1] = y - dn[1, yi, xi]
    return kp2


def _kp_elastic(kp, params, H, W):
    return _elastic_keypoints(kp, elastic_shift(params, H, W), H, W)


def _px_gaussian_noise(img, params):
    noise = params["field"]
    if noise is None:
        raise ValueError("this plan's noise is a device key (noise=\"key\"); the host applies plans built with noise=\"field\"")
    out = img.astype(np.float32) + np.float32(params["scale"]) * noise
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def crop_amounts(top, right, bottom, left, H, W):
    """CropAndPad's fractions of the frame per side -> whole rows / columns (top, right, bottom, left): < 0 crops, > 0 pads"""
    t, b = int(round(top * H)), int(round(bottom * H))
    l, r = int(round(left * W)), int(round(right * W))
    # never crop the image away (imgaug keeps at least one pixel per axis)
    if -(t + b) >= H:
        t = b = -((H - 1) // 2)
    if -(l + r) >= W:
        l = r = -((W - 1) // 2)
    return t, r, b, l


def crop_geometry(params, H, W):
    """-> (x0, x1, y0, y1, pt, pb, pl, pr): the core img[y0:y1, x0:x1] and the zero rows / columns around it, before the resize back"""
    t, r, b, l = params["amounts"]
    x0, x1 = max(0, -l), W - max(0, -r)
    y0, y1 = max(0, -t), H - max(0, -b)
    return x0, x1, y0, y1, max(0, t), max(0, b), max(0, l), max(0, r)


def _px_crop_and_pad(img, params):
    from PIL import Image
    H, W = img.shape[:2]
    x0, x1, y0, y1, pt, pb, pl_, pr = crop_geometry(params, H, W)
    core = np.pad(img[y0:y1, x0:x1], ((pt, pb), (pl_, pr), (0, 0)), mode="constant")
    return np.asarray(Image.fromarray(core).resize((W, H), Image.BILINEAR))    # keep_size=True


def _kp_crop_and_pad(kp, params, H, W):
    x0, x1, y0, y1, pt, pb, pl_, pr = crop_geometry(params, H, W)
    w2, h2 = (x1 - x0) + pl_ + pr, (y1 - y0) + pt + pb
    kp2 = kp.copy()
    kp2[:, 0] = (kp[:, 0] - x0 + pl_) * (W / float(w2))
    kp2[:, 1] = (kp[:, 1] - y0 + pt) * (H / float(h2))
    return kp2


_PIXELS = {"fliplr": _px_fliplr, "rotate": _px_rotate, "motion_blur": _px_motion_blur, "coarse_dropout": _px_coarse_dropout,
           "gaussian_noise": _px_gaussian_noise, "crop_and_pad": _px_crop_and_pad}
_KEYPOINTS = {"fliplr": _kp_fliplr, "rotate": _kp_rotate, "motion_blur": _kp_same, "coarse_dropout": _kp_same, "elastic": _kp_elastic,
              "gaussian_noise": _kp_same, "crop_and_pad": _kp_crop_and_pad}


def _apply(stage, img, kp, params):
    H, W = img.shape[:2]
    if stage == "elastic":                                            # (not in _PIXELS: one upsampling of the field serves both halves)
        d = elastic_shift(params, H, W)
        return _elastic_pixels(img, d), _elastic_keypoints(kp, d, H, W)
    return _PIXELS[stage](img, params), _KEYPOINTS[stage](kp, params, H, W)


def apply_fliplr(img, kp, params):
    return _apply("fliplr", img, kp, params)


def apply_rotate(img, kp, params):
    return _apply("rotate", img, kp, params)


def apply_motion_blur(img, kp, params):
    return _apply("motion_blur", img, kp, params)


def apply_coarse_dropout(img, kp, params):
    return _apply("coarse_dropout", img, kp, params)


def apply_elastic(img, kp, params):
    """ElasticTransformation(sigma=5, alpha=(0, 10)): out[p] = in[p + d(p)], d = alpha * gaussian_filter(uniform(-1, 1), sigma).
    With sigma = 5 the field is smooth over tens of pixels, so it is synthesised on a grid of every 4th pixel -- white noise of
    variance (1/3) / 16 filtered with sigma / 4: the same variance and correlation length as the full-resolution field -- and
    brought to full resolution bilinearly; the resampling (bilinear, zeros outside: imgaug's order 1 / cval 0) is torch's
    multi-threaded CPU grid_sample instead of one scipy map_coordinates per channel (100 -> 8 ms on a 640 x 480 frame)."""
    return _apply("elastic", img, kp, params)


def apply_gaussian_noise(img, kp, params):
    return _apply("gaussian_noise", img, kp, params)


def apply_crop_and_pad(img, kp, params):
    return _apply("crop_and_pad", img, kp, params)


def keypoints_of(plan, kp, H, W):
    """The keypoint half of apply_host alone (the same functions): where a plan moves the (x, y) keypoints `kp` [nj, 2] of an H x W frame"""
    kp = np.asarray(kp, dtype=np.float64).reshape(-1, 2)
    for stage, params in plan:
        kp = _KEYPOINTS[stage](kp, params, H, W)
    return kp


def plan_stages(plans):
    """{stage: how many of `plans` hold it}, every stage named"""
    count = dict.fromkeys(STAGES, 0)
    for plan in plans:
        for stage, _ in plan:
            count[stage] += 1
    return count


class NumpyAugPipeline:
    def __init__(self, apply_prob: float = 0.5, seed=None):
        self.p = float(apply_prob)
        if seed is None:        # reproducible under np.random.seed(...) like the rest of the fit drivers' schedule (not OS entropy)
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.rng = np.random.RandomState(seed)
        self.bulk = np.random.Generator(np.random.PCG64(int(self.rng.randint(0, 2 ** 31 - 1))))      # per-pixel noise fields, device keys
        self.last_plans = []    # the plans of the last __call__, one per image
        # the elastic warp runs on torch's CPU thread pool, from the fit drivers' prefetch thread, next to the thread that feeds the
        # GPU: on a 256-core host an unbounded pool (and its spinning idle workers) halves the launch rate of the training step.
        # A frame needs no more than a few cores.
        try:
            import torch
            if torch.get_num_threads() > 8:
                torch.set_num_threads(8)
        except ImportError:
            pass

    # ---- the draws of the seven augmenters: (H, W) -> params.  They alone consume self.rng / self.bulk ----
    def draw_fliplr(self, H, W):
        return {"flip": bool(self.rng.random_sample() < 0.5)}

    def draw_rotate(self, H, W):
        deg = self.rng.uniform(-10, 10)
        return {"deg": deg, "coef": rotate_coefficients(deg, H, W)[0]}

    def draw_motion_blur(self, H, W):
        return {"kernel": motion_blur_kernel(self.rng.uniform(-90, 90))}

    def draw_coarse_dropout(self, H, W):
        p = self.rng.uniform(0, 0.02)
        sp = self.rng.uniform(0.01, 0.05)
        h, w = max(1, int(round(H * sp))), max(1, int(round(W * sp)))
        return {"mask": self.rng.random_sample((h, w)) < p}

    def draw_elastic(self, H, W):
        from scipy import ndimage
        alpha = self.rng.uniform(0, 10)
        S = ELASTIC_STEP
        hc, wc = -(-(H - 1) // S) + 1, -(-(W - 1) // S) + 1               # node (i, j) sits on pixel (S i, S j); the last node at or past the edge
        dxc = ndimage.gaussian_filter((self.rng.random_sample((hc, wc)) * 2 - 1) / S, 5.0 / S, mode="constant") * alpha
        dyc = ndimage.gaussian_filter((self.rng.random_sample((hc, wc)) * 2 - 1) / S, 5.0 / S, mode="constant") * alpha
        return {"alpha": alpha, "field": np.stack([dxc, dyc]).astype(np.float32)}

    def draw_gaussian_noise(self, H, W, noise="field"):
        """noise "field": the per-pixel standard normal field the host adds, drawn from self.bulk (4x faster than RandomState.normal);
        "key": one uint64 from self.bulk instead, the key of the device's counter-based generator.  self.rng is consumed alike."""
        if noise not in NOISE_SOURCES:
            raise ValueError("noise must be one of %s, not %r" % (" | ".join(NOISE_SOURCES), noise))
        scale = self.rng.uniform(0.0, 0.01 * 255)
        per_channel = bool(self.rng.random_sample() < 0.5)
        if noise == "key":
            return {"scale": scale, "per_channel": per_channel, "field": None, "key": int(self.bulk.integers(0, 2 ** 64, dtype=np.uint64))}
        field = self.bulk.standard_normal(size=(H, W, 3 if per_channel else 1), dtype=np.float32)
        return {"scale": scale, "per_channel": per_channel, "field": field, "key": None}

    def draw_crop_and_pad(self, H, W):
        top, right, bottom, left = self.rng.uniform(-0.3, 0.1, size=4)    # one draw per side; < 0 crops, > 0 pads (zeros)
        return {"amounts": crop_amounts(top, right, bottom, left, H, W)}

    # ---- the seven augmenters: (image uint8 [H,W,C], keypoints float [nj,2] as (x, y)) -> the same; draw, then apply ----
    def fliplr(self, img, kp):
        return apply_fliplr(img, kp, self.draw_fliplr(*img.shape[:2]))

    def rotate(self, img, kp):
        return apply_rotate(img, kp, self.draw_rotate(*img.shape[:2]))

    def motion_blur(self, img, kp):
        return apply_motion_blur(img, kp, self.draw_motion_blur(*img.shape[:2]))

    def coarse_dropout(self, img, kp):
        return apply_coarse_dropout(img, kp, self.draw_coarse_dropout(*img.shape[:2]))

    def elastic(self, img, kp):
        return apply_elastic(img, kp, self.draw_elastic(*img.shape[:2]))

    def gaussian_noise(self, img, kp):
        return apply_gaussian_noise(img, kp, self.draw_gaussian_noise(*img.shape[:2]))

    def crop_and_pad(self, img, kp):
        return apply_crop_and_pad(img, kp, self.draw_crop_and_pad(*img.shape[:2]))

    # ---- a frame's augmentation as a plan ----
    def plan(self, H, W, noise="field"):
        """Draw one H x W frame's augmentation: [(stage, params), ...] of the stages whose Sometimes coin came up, in pipeline order.
        Consumes self.rng exactly as augmenting the frame does; `noise` as in draw_gaussian_noise."""
        if noise not in NOISE_SOURCES:
            raise ValueError("noise must be one of %s, not %r" % (" | ".join(NOISE_SOURCES), noise))
        H, W = int(H), int(W)
        plan = []
        for stage in STAGES:
            if self.rng.random_sample() < (0.4 if stage == "crop_and_pad" else self.p):
                draw = getattr(self, "draw_" + stage)
                plan.append((stage, draw(H, W, noise) if stage == "gaussian_noise" else draw(H, W)))
        return plan

    def apply_host(self, plan, img, kp):
        """Apply a plan (built with noise="field") to one image and its keypoints on the host -> (img, kp).  An augmenter replaced on
        the instance (pipeline.crop_and_pad = ...) is called in place of the planned stage, as __call__ always did."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        kp = np.asarray(kp, dtype=np.float64).reshape(-1, 2)
        for stage, params in plan:
            if stage in self.__dict__:
                img, kp = self.__dict__[stage](img, kp)
            else:
                img, kp = _apply(stage, img, kp, params)
        return img, kp

    def __call__(self, images, keypoints):
        out_imgs, out_kps = [], []
        self.last_plans = []
        for img, kps in zip(images, keypoints):
            plan = self.plan(img.shape[0], img.shape[1], "field")
            self.last_plans.append(plan)
            img, kp = self.apply_host(plan, img, kps)
            out_imgs.append(np.ascontiguousarray(img))
            out_kps.append([tuple(v) for v in kp.tolist()])
        return np.stack(out_imgs), out_kps


def build_aug(apply_prob: float = 0.5, seed=None, backend: str = "auto"):
    """The reference's pipeline (fitdgp_util.py:412-436).  backend: 'imgaug' | 'numpy' | 'auto' (imgaug if importable)."""
    if backend in ("auto", "imgaug"):
        try:
            import imgaug.augmenters as iaa
        except ImportError:
            if backend == "imgaug":
                raise
        else:
            sometimes = lambda aug: iaa.Sometimes(apply_prob, aug)
            pipeline = iaa.Sequential(random_order=False)
            pipeline.add(sometimes(iaa.Fliplr(0.5)))
            pipeline.add(sometimes(iaa.Affine(rotate=(-10, 10))))
            pipeline.add(sometimes(iaa.MotionBlur(k=3, angle=(-90, 90))))
            pipeline.add(sometimes(iaa.CoarseDropout((0, 0.02), size_percent=(0.01, 0.05))))
            pipeline.add(sometimes(iaa.ElasticTransformation(sigma=5, alpha=(0, 10))))
            pipeline.add(sometimes(iaa.AdditiveGaussianNoise(loc=0, scale=(0.0, 0.01 * 255), per_channel=0.5)))
            pipeline.add(iaa.Sometimes(0.4, iaa.CropAndPad(percent=(-0.3, 0.1), keep_size=True)))
            return pipeline
    return NumpyAugPipeline(apply_prob, seed)


def _labels_to_keypoints(joint_loc, stride):
    """labels (row, col) in scoremap cells -> (x, y) px, float64 [n, nj, 2]"""
    return np.flip(np.asarray(joint_loc, dtype=np.float64), 2) * stride + stride / 2


def _keypoints_to_labels(keypoints, stride):
    return np.flip(np.array(keypoints, dtype=np.float64) / stride - 0.5, 2)


def data_aug(all_data_batch, visible_frame_within_batch, joint_loc, pipeline, dgp_cfg):
    """fitdgp_util.py:439-451: augment the visible frames; labels (row, col) in scoremap cells <-> (x, y) px."""
    stride = float(dgp_cfg.stride)
    visible_data = all_data_batch[visible_frame_within_batch, :, :, :].astype(np.uint8)
    xy = _labels_to_keypoints(joint_loc, stride)
    kp_list = [[tuple(f) for f in v.tolist()] for v in xy]
    batch_images, batch_joints = pipeline(images=visible_data, keypoints=kp_list)
    joint_loc_aug = _keypoints_to_labels(batch_joints, stride)
    all_data_batch_aug = np.copy(all_data_batch)
    all_data_batch_aug[visible_frame_within_batch, :, :, :] = np.asarray(batch_images)
    return all_data_batch_aug, joint_loc_aug


def plan_aug(n, H, W, joint_loc, pipeline, dgp_cfg):
    """data_aug's draws and labels without its pixels: one plan(H, W, "key") per visible frame, in data_aug's order, and the labels
    moved by keypoints_of through data_aug's own flips and stride arithmetic -> (plans, joint_loc_aug).  The pixels are then
    engine.augment_frames' to make."""
    stride = float(dgp_cfg.stride)
    xy = _labels_to_keypoints(joint_loc, stride)
    plans = [pipeline.plan(H, W, "key") for _ in range(int(n))]
    moved = [keypoints_of(plan, kp, H, W) for plan, kp in zip(plans, xy)]
    return plans, _keypoints_to_labels(moved, stride)
