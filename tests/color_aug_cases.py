"""Cases shared by the colour tests (CPU and GPU) and by tests/golden/gen_color_aug_golden.py: sources, operation
lists and views, all deterministic.  Nothing here depends on the code under test beyond the ColorAug / View records."""
import numpy as np

from bm2f_amd import ColorAug, View

MEAN, STD = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]
SWEEP_B = (0, 1, 127, 128, 254, 255)
SWEEP_STRIDE = 8           # the fixture keeps every 8th row and column of a sweep output


def sweep_image():
    """All (r, g) pairs at b in SWEEP_B as a 256 x 1536 BGR image: row r, column 256 * i + g."""
    r, g = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.ascontiguousarray(np.concatenate([np.stack([np.full_like(r, b), g, r], -1) for b in SWEEP_B],
                                               axis=1).astype(np.uint8))


def random_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# each single SSD step at its edge values, both full orders (BGR and RGB), each video blend and the video chain
COLOR_CASES = {
    "ssd_brightness_p32": ColorAug((("ssd_brightness", 32.0),)),
    "ssd_brightness_m": ColorAug((("ssd_brightness", -17.3),)),
    "ssd_contrast_05": ColorAug((("ssd_contrast", 0.5),)),
    "ssd_contrast_15": ColorAug((("ssd_contrast", 1.5),)),
    "ssd_saturation_05": ColorAug((("ssd_saturation", 0.5),)),
    "ssd_saturation_137": ColorAug((("ssd_saturation", 1.37),)),
    "ssd_hue_p18": ColorAug((("ssd_hue", 18),)),
    "ssd_hue_m18": ColorAug((("ssd_hue", -18),)),
    "ssd_order_a": ColorAug((("ssd_brightness", -9.25), ("ssd_contrast", 1.21), ("ssd_saturation", 0.77),
                             ("ssd_hue", 11))),
    "ssd_order_b_rgb": ColorAug((("ssd_brightness", 20.5), ("ssd_saturation", 1.3), ("ssd_hue", -7),
                                 ("ssd_contrast", 0.83)), swap_rb=True),
    "video_brightness": ColorAug((("brightness", 0.9),)),
    "video_contrast": ColorAug((("contrast", 1.1),)),
    "video_saturation_09": ColorAug((("saturation", 0.9),)),
    "video_saturation_11": ColorAug((("saturation", 1.1),)),
    "video_all": ColorAug((("brightness", 1.0731), ("contrast", 0.9412), ("saturation", 1.0517))),
}
FAMILIES = ("ssd_order_a", "ssd_order_b_rgb", "video_all", "ssd_hue_m18")

# geometry: a 37 x 53 source, smaller and larger, crop past the image, both flips, a canvas wider than a 64-column tile
GEO_SOURCE = (37, 53)
GEO_VIEWS = {
    "down_crop_past_flip_out": dict(size=(23, 31), crop=(-3, 5, 30, 40), canvas=(40, 70), flip_out=True, fill=128),
    "down_flip_in": dict(size=(23, 31), crop=(4, -6, 17, 33), canvas=(17, 33), flip_in=True, fill=128),
    "up_wide_canvas": dict(size=(61, 89), crop=(10, 7, 60, 90), canvas=(64, 96), flip_in=True, flip_out=True, fill=128),
    "up_whole": dict(size=(61, 89), fill=128),
}
GEO_PAD = 32               # size_divisibility of the geometry calls


def geo_view(name, color, source=0):
    return View(source=source, color=color, **GEO_VIEWS[name])


# contrast mean: one pixel, 3 x 5 pixels and a view of several workgroups (61 x 89: two column tiles, four row tiles)
MEAN_CASES = {
    "one_pixel": ((5, 7), View(size=(1, 1))),
    "three_by_five": ((3, 5), View(size=(3, 5))),
    "several_workgroups": (GEO_SOURCE, View(size=(61, 89), crop=(-2, -3, 70, 100), canvas=(70, 100), fill=128)),
}
MEAN_AUGS = {
    "contrast_first": ColorAug((("contrast", 0.9),)),
    "contrast_after": ColorAug((("brightness", 1.1), ("contrast", 1.1), ("saturation", 0.9))),
    "contrast_after_hue": ColorAug((("ssd_hue", 9), ("contrast", 0.95))),
}


def literal_blends(img, w):
    """detectron2's ``BlendTransform.apply_image`` for the three video augmentations, written as its source writes it."""
    def blend(src_image, src_weight, dst_weight):
        x = img.astype(np.float32)
        x = src_weight * src_image + dst_weight * x
        return np.clip(x, 0, 255).astype(np.uint8)
    return {"brightness": blend(0, 1 - w, w), "contrast": blend(img.mean(), 1 - w, w),
            "saturation": blend(img.dot([0.299, 0.587, 0.114])[:, :, np.newaxis], 1 - w, w)}


def literal_convert(img, alpha=1, beta=0):
    """``ColorAugSSDTransform.convert`` as its source writes it."""
    x = img.astype(np.float32) * alpha + beta
    x = np.clip(x, 0, 255)
    return x.astype(np.uint8)
