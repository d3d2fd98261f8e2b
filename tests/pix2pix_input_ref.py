"""float64 NumPy restatement of the Pix2Pix input pipeline of the reference (Pix2Pix/train.py:135-271, 355-431, 627-633), written
from its formulae for the tests of gank_pix2pix_load_examples / gank_rgb_to_lab / gank_lab_to_rgb / gank_pix2pix_convert_u8.
The reference itself needs TensorFlow 1.x and cannot run here; tests/test_pix2pix_input_cpu.py pins this file by known answers
that do not depend on it (mean pooling, nearest neighbour, the Lab values of the primaries, the round trip)."""
import numpy as np

MODES = {"pair": 0, "multiple_A": 1, "lab_colorization": 2}


def preprocess(x):                      # train.py:135-138
    return x * 2 - 1


def deprocess(x):                       # train.py:141-144
    return (x + 1) / 2


def rgb_to_lab(srgb):
    """train.py:178-218, [..., 3] in [0, 1]"""
    s = np.asarray(srgb, np.float64)
    px = s.reshape(-1, 3)
    lin, ex = (px <= 0.04045).astype(np.float64), (px > 0.04045).astype(np.float64)
    rgb = (px / 12.92 * lin) + (((px + 0.055) / 1.055) ** 2.4) * ex
    m = np.array([[0.412453, 0.212671, 0.019334], [0.357580, 0.715160, 0.119193], [0.180423, 0.072169, 0.950227]])
    xyz = rgb @ m
    xyz = xyz * np.array([1 / 0.950456, 1.0, 1 / 1.088754])
    eps = 6 / 29
    lin, ex = (xyz <= eps ** 3).astype(np.float64), (xyz > eps ** 3).astype(np.float64)
    f = (xyz / (3 * eps ** 2) + 4 / 29) * lin + (xyz ** (1 / 3)) * ex
    m2 = np.array([[0.0, 500.0, 0.0], [116.0, -500.0, 200.0], [0.0, 0.0, -200.0]])
    return (f @ m2 + np.array([-16.0, 0.0, 0.0])).reshape(s.shape)


def lab_to_rgb(lab):
    """train.py:221-262"""
    s = np.asarray(lab, np.float64)
    px = s.reshape(-1, 3)
    m = np.array([[1 / 116.0, 1 / 116.0, 1 / 116.0], [1 / 500.0, 0.0, 0.0], [0.0, 0.0, -1 / 200.0]])
    f = (px + np.array([16.0, 0.0, 0.0])) @ m
    eps = 6 / 29
    lin, ex = (f <= eps).astype(np.float64), (f > eps).astype(np.float64)
    xyz = (3 * eps ** 2 * (f - 4 / 29)) * lin + (f ** 3) * ex
    xyz = xyz * np.array([0.950456, 1.0, 1.088754])
    m2 = np.array([[3.2404542, -0.9692660, 0.0556434], [-1.5371385, 1.8760108, -0.2040259], [-0.4985314, 0.0415560, 1.0572252]])
    rgb = np.clip(xyz @ m2, 0.0, 1.0)
    lin, ex = (rgb <= 0.0031308).astype(np.float64), (rgb > 0.0031308).astype(np.float64)
    return ((rgb * 12.92 * lin) + ((rgb ** (1 / 2.4) * 1.055) - 0.055) * ex).reshape(s.shape)


def preprocess_lab(lab):                # train.py:147-153
    return lab[..., 0] / 50 - 1, lab[..., 1] / 110, lab[..., 2] / 110


def deprocess_lab(L, a, b):             # train.py:156-159
    return np.stack([(L + 1) / 2 * 100, a * 110, b * 110], axis=-1)


def augment(ab, brightness):            # train.py:265-271
    return lab_to_rgb(deprocess_lab(brightness[..., 0], ab[..., 0], ab[..., 1]))


def area_weights(n_in, n_out):
    """[n_out, n_in]: the length of the overlap of source cell [i, i+1) with the span [y*s, (y+1)*s), s = n_in / n_out, of output
    y (tf.image.resize_images, ResizeMethod.AREA; indices clamped to the image), not yet divided by s"""
    s = n_in / n_out
    w = np.zeros((n_out, n_in))
    for y in range(n_out):
        lo, hi = y * s, (y + 1) * s
        for i in range(int(np.floor(lo)), int(np.ceil(hi))):
            w[y, min(max(i, 0), n_in - 1)] += max(0.0, min(hi, i + 1) - max(lo, i))
    return w


def area_resize(img, out_h, out_w):
    """[H, W, C] -> [out_h, out_w, C]: the weighted sums over both axes divided by s_y * s_x"""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    wy, wx = area_weights(h, out_h), area_weights(w, out_w)
    rows = np.tensordot(wy, img, axes=(1, 0))                       # [out_h, W, C]
    return np.einsum("xj,yjc->yxc", wx, rows, optimize=True) / ((h / out_h) * (w / out_w))


def split_frame(frame, mode):
    """one uint8 [H, W, 3] frame -> (a_image, b_image) float64 after convert_image_dtype and preprocess / Lab (train.py:355-396)"""
    x = np.asarray(frame, np.float64) / 255.0
    w = x.shape[1]
    if mode == 2:
        L, a, b = preprocess_lab(rgb_to_lab(x))
        return L[..., None], np.stack([a, b], axis=-1)
    if mode == 1:
        assert w % 3 == 0
        p = w // 3
        return np.concatenate([preprocess(x[:, :p]), preprocess(x[:, p:2 * p])], axis=2), preprocess(x[:, 2 * p:])
    assert w % 2 == 0
    return preprocess(x[:, :w // 2]), preprocess(x[:, w // 2:])


def transform(img, flip, scale_h, scale_w, crop, oy, ox):      # train.py:408-423
    if flip:
        img = img[:, ::-1]
    r = area_resize(img, scale_h, scale_w)
    assert scale_h >= crop and scale_w >= crop and 0 <= oy <= scale_h - crop and 0 <= ox <= scale_w - crop
    return r[oy:oy + crop, ox:ox + crop]


def load_examples(raw, mode, direction, scale_h, scale_w, crop, table):
    """raw uint8 [N,H,W,3], table [N,3] (flip, offset_y, offset_x) -> (inputs, targets) float64 [N,crop,crop,C]"""
    ins, tgs = [], []
    for frame, (flip, oy, ox) in zip(raw, np.asarray(table)):
        a, b = split_frame(frame, mode)
        a, b = (transform(t, flip, scale_h, scale_w, crop, int(oy), int(ox)) for t in (a, b))
        ins.append(a if direction == 0 else b)
        tgs.append(b if direction == 0 else a)
    return np.stack(ins), np.stack(tgs)


def convert01(x01):
    """tf.image.convert_image_dtype(uint8, saturate=True) of an image in [0, 1] (train.py:633): scale by max + 0.5, saturate, truncate"""
    return np.trunc(np.clip(np.asarray(x01, np.float64) * 255.5, 0.0, 255.0)).astype(np.uint8)


def convert_u8(x):
    """deprocess + convert of an image in [-1, 1]"""
    return convert01(deprocess(np.asarray(x, np.float64)))
