"""Shared plumbing of the JPEG-size tests: Pillow as the reference encoder, a reader of the marker segments of the files it writes,
and the test images."""
import io

import numpy as np

# natural (row-major) index of the k-th coefficient of the zigzag sequence (ITU T.81 figure A.6)
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def pil_jpeg(img, quality=80):
    """bytes of the file the compressibility reward measures: img uint8 [3, h, w] -> PIL.Image.save(format='JPEG', quality=quality)"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(np.transpose(img, (1, 2, 0)))).save(buf, format='JPEG', quality=quality)
    return buf.getvalue()


def parse_segments(data):
    """{'dqt': {table id: 64 entries, natural order}, 'entropy': offset of the entropy-coded data} of a baseline JPEG file"""
    assert data[:2] == b'\xff\xd8'
    out, p = dict(dqt={}), 2
    while True:
        assert data[p] == 0xFF, p
        marker, length = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + length]
        if marker == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0                      # 8-bit entries
                table = [0] * 64
                for k in range(64):
                    table[ZIGZAG[k]] = seg[1 + k]
                out['dqt'][seg[0] & 15] = table
                seg = seg[65:]
        p += 2 + length
        if marker == 0xDA:
            out['entropy'] = p
            return out


def make_images(kind, n, h, w, seed=0):
    """n distinct uint8 images [n, 3, h, w]: 'noise' uniform, 'smooth' a low-frequency wave plus a little noise, 'flat' one grey level per
    image, 'sat' random 0 / 255 (the largest coefficients, the longest codes)"""
    g = np.random.default_rng([seed, n, h, w])
    if kind == 'noise':
        return g.integers(0, 256, (n, 3, h, w)).astype(np.uint8)
    if kind == 'sat':
        return (g.integers(0, 2, (n, 3, h, w)) * 255).astype(np.uint8)
    if kind == 'flat':
        return np.broadcast_to(((np.arange(n) * 37 + 5) % 256).astype(np.uint8)[:, None, None, None], (n, 3, h, w)).copy()
    assert kind == 'smooth'
    yy, xx = np.mgrid[0:h, 0:w]
    ph = g.uniform(0, 6.28, (n, 3, 1, 1))
    wave = 128 + 100 * np.sin(xx / 9.0 + ph) * np.cos(yy / 7.0 + ph)
    return np.clip(wave + g.normal(0, 4, (n, 3, h, w)), 0, 255).astype(np.uint8)


def zrl_image():
    """One 16x16 MCU whose blocks hold the DC coefficient and (a multiple of) the highest-frequency basis function only: in every Y block
    a zero run longer than 15 stands in front of a non-zero coefficient, the chroma blocks have the single AC coefficient 63 (a run of
    62: three ZRL codes), and every block ends on coefficient 63 (no EOB)."""
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    b8 = np.outer(k, k)
    grey = 128 + 50 * np.tile(b8, (2, 2))
    img = np.stack([grey, grey, grey + 70 * np.kron(b8, np.ones((2, 2)))])
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
