"""Shared plumbing of the JPEG-size tests: Pillow as the reference encoder, a reader of the marker segments of the files it writes, a
baseline entropy decoder of those files (the reference of every stage of the HIP path: coefficients, block bit offsets, the bit stream),
the test images, and the transform stage as an integer numpy model."""
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
    """{'dqt': {table id: 64 entries, natural order}, 'entropy': offset of the entropy-coded data, 'dht': {(class, id): (16 counts, symbols)},
    'sof': (height, width, [(component id, h factor, v factor, quantisation table)]), 'sos': [(component id, DC table, AC table)]} of a
    baseline JPEG file"""
    assert data[:2] == b'\xff\xd8'
    out, p = dict(dqt={}, dht={}), 2
    while True:
        assert data[p] == 0xFF, p
        marker, length = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + length]
        assert marker not in (0xC1, 0xC2, 0xC3, 0xC9, 0xCA, 0xCB, 0xDD), f'marker {marker:#x}: not a baseline file without restarts'
        if marker == 0xC4:
            while seg:
                counts = list(seg[1:17])
                out['dht'][(seg[0] >> 4, seg[0] & 15)] = (counts, list(seg[17:17 + sum(counts)]))
                seg = seg[17 + sum(counts):]
        if marker == 0xC0:
            assert seg[0] == 8                               # sample precision
            out['sof'] = ((seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4],
                          [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])])
        if marker == 0xDA:
            out['sos'] = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
            assert tuple(seg[1 + 2 * seg[0]:]) == (0, 63, 0)  # one sequential scan of whole coefficients
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


SPECIAL_KINDS = ['checker', 'redblue', 'ac10', 'ac10c', 'zrl']


def special_image(kind, h, w):
    """uint8 [3, h, w] (h, w multiples of 16), built to reach the largest categories at quality 100:
    'checker' 8x8 blocks alternately black and white: successive luma DC values swing over the whole range (difference category 11);
    'redblue' 16x16 MCUs alternately saturated red and saturated blue: the same for the Cb and Cr DC values;
    'ac10'    grey; every 8x8 block is the SIGN of the highest-frequency basis function, 0 / 255: the largest single AC coefficient an
              8-bit image gives (category 10), at position 63 of every luma block;
    'ac10c'   the same pattern at half the resolution in blue and its complement in red and green: Cb swings over its whole range, so the
              category-10 coefficient stands in the chroma blocks;
    'zrl'     zrl_image tiled (runs of 62 = three ZRL codes in front of coefficient 63; at qualities up to 30 in both tables)."""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'checker':
        g = (((yy >> 3) + (xx >> 3)) & 1) * 255
        return np.stack([g, g, g]).astype(np.uint8)
    if kind == 'redblue':
        red = (((yy >> 4) + (xx >> 4)) & 1) == 0
        return np.stack([np.where(red, 255, 0), np.zeros((h, w), dtype=np.int64), np.where(red, 0, 255)]).astype(np.uint8)
    if kind == 'zrl':
        return np.tile(zrl_image(), (1, h // 16, w // 16))
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    sign = np.where(np.outer(k, k) > 0, 255, 0)
    if kind == 'ac10':
        g = np.tile(sign, (h // 8, w // 8))
        return np.stack([g, g, g]).astype(np.uint8)
    assert kind == 'ac10c'
    p = np.tile(np.kron(sign, np.ones((2, 2), dtype=np.int64)), (h // 16, w // 16))
    return np.stack([255 - p, 255 - p, p]).astype(np.uint8)


def all_kinds(h, w, seed=0):
    """(names, uint8 [9, 3, h, w]): one image of every kind of make_images and of every special kind"""
    names = ['noise', 'smooth', 'flat', 'sat'] + SPECIAL_KINDS
    imgs = [make_images(k, 1, h, w, seed=seed)[0] for k in names[:4]] + [special_image(k, h, w) for k in SPECIAL_KINDS]
    return names, np.stack(imgs)


# ---- a baseline entropy decoder: what the file Pillow wrote says, stage by stage -----------------------------------------------------------
class Scan:
    """What decode_scan reads off one file.  Per-table entries are indexed by the Huffman table id (0: luma, 1: chroma)."""
    __slots__ = ('height', 'width', 'header', 'coef', 'start', 'total', 'stream', 'stuffed', 'dc_cat', 'ac_cat', 'lane', 'run', 'no_eob')


def _decode_table(counts, symbols):
    """16-bit prefix -> (symbol, code length) of a DHT segment's table (T.81 Annex C: codes of one length are consecutive, the first of
    the next length is the successor doubled); 0 length = no code has this prefix"""
    sym, ln = np.zeros(65536, dtype=np.int32), np.zeros(65536, dtype=np.int32)
    code = k = 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            lo = code << (16 - length)
            sym[lo:lo + (1 << (16 - length))] = symbols[k]
            ln[lo:lo + (1 << (16 - length))] = length
            code, k = code + 1, k + 1
        code <<= 1
    return sym.tolist(), ln.tolist()


def decode_scan(data):
    """Entropy-decode the baseline, 4:2:0, single-scan JPEG file `data` with the Huffman tables of its own DHT segments.  Returns a Scan:
    coef    int16 [blocks, 64]: quantised coefficients, zigzag, blocks in scan order (per MCU: four Y, Cb, Cr), DC de-differenced
    start   int64 [blocks]: first bit of every block in the unstuffed stream;  total: bits up to the end of the last block
    stream  the entropy-coded bytes without the stuffed zeros;  stuffed: FF 00 pairs removed;  header: bytes in front of the stream
    dc_cat, ac_cat, lane, run: per Huffman table id, the largest DC difference category, the largest AC category, the longest single AC
            contribution in bits (ZRL codes + run/size code + value bits) and the longest zero run in front of a coefficient
    no_eob  blocks that end on coefficient 63
    Asserts that fewer than 8 bits follow the last block and that all of them are ones."""
    seg = parse_segments(data)
    out = Scan()
    out.height, out.width, comps = seg['sof']
    assert [(c[1], c[2]) for c in comps] == [(2, 2), (1, 1), (1, 1)], comps          # 4:2:0
    assert [c[0] for c in comps] == [c[0] for c in seg['sos']]
    assert data[-2:] == b'\xff\xd9'
    out.header = seg['entropy']
    raw = data[seg['entropy']:-2]
    out.stuffed = raw.count(b'\xff\x00')
    out.stream = raw.replace(b'\xff\x00', b'\xff')
    assert out.stream.count(b'\xff') == out.stuffed, 'a marker inside the scan'
    # 32-bit big-endian window at every byte: bits [8 b, 8 b + 32) of the stream, ones past its end
    padded = np.frombuffer(out.stream + b'\xff' * 4, dtype=np.uint8).astype(np.int64)
    win = ((padded[:-3] << 24) | (padded[1:-2] << 16) | (padded[2:-1] << 8) | padded[3:]).tolist()
    tables = {key: _decode_table(*val) for key, val in seg['dht'].items()}
    plan = []                                                # per block of an MCU: (component, DC table id, AC table id)
    for ci, (_, hf, vf, _) in enumerate(comps):
        plan += [(ci, seg['sos'][ci][1], seg['sos'][ci][2])] * (hf * vf)
    mcus = ((out.height + 15) // 16) * ((out.width + 15) // 16)
    coef = np.zeros((mcus * len(plan), 64), dtype=np.int16)
    start = np.zeros(mcus * len(plan), dtype=np.int64)
    out.dc_cat, out.ac_cat, out.lane, out.run, out.no_eob = [0, 0], [0, 0], [0, 0], [0, 0], 0
    pred, pos, b = [0] * len(comps), 0, 0
    for _ in range(mcus):
        for ci, td, ta in plan:
            start[b] = pos
            row = coef[b]
            dsym, dlen = tables[(0, td)]
            peek = (win[pos >> 3] >> (16 - (pos & 7))) & 0xFFFF
            size, n = dsym[peek], dlen[peek]
            assert n > 0, (b, pos)
            pos += n
            diff = 0
            if size:
                diff = (win[pos >> 3] >> (32 - size - (pos & 7))) & ((1 << size) - 1)
                if diff < (1 << (size - 1)):
                    diff -= (1 << size) - 1
                pos += size
            out.dc_cat[td] = max(out.dc_cat[td], size)
            pred[ci] += diff
            row[0] = pred[ci]
            asym, alen = tables[(1, ta)]
            k, run, lane = 1, 0, 0
            while k < 64:
                peek = (win[pos >> 3] >> (16 - (pos & 7))) & 0xFFFF
                rs, n = asym[peek], alen[peek]
                assert n > 0, (b, k, pos)
                pos += n
                lane += n
                if rs == 0:                                  # EOB
                    break
                if rs == 0xF0:                               # ZRL
                    k, run = k + 16, run + 16
                    continue
                r, size = rs >> 4, rs & 15
                k, run = k + r, run + r
                assert size and k < 64, (b, k, rs)
                v = (win[pos >> 3] >> (32 - size - (pos & 7))) & ((1 << size) - 1)
                if v < (1 << (size - 1)):
                    v -= (1 << size) - 1
                pos += size
                row[k] = v
                out.ac_cat[ta] = max(out.ac_cat[ta], size)
                out.lane[ta] = max(out.lane[ta], lane + size)
                out.run[ta] = max(out.run[ta], run)
                k, run, lane = k + 1, 0, 0
            else:
                assert k == 64 and run == 0, (b, k, run)     # a ZRL never ends a block
                out.no_eob += 1
            b += 1
    out.coef, out.start, out.total = coef, start, pos
    tail = 8 * len(out.stream) - pos
    assert 0 <= tail < 8, (tail, pos, len(out.stream))
    assert tail == 0 or out.stream[-1] & ((1 << tail) - 1) == (1 << tail) - 1, 'the padding bits are not all ones'
    return out


def stream_bits(data, total=None):
    """uint8 array of the bits of `data` (bytes), first bit of the stream first; the first `total` of them"""
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8))
    return bits if total is None else bits[:total]


# ---- the transform stage as an integer numpy model --------------------------------------------------------------------------------------
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def model_fdct(b):
    """the "slow integer" 8x8 forward DCT over the last two axes of an int64 array: 13-bit constants, 2 extra bits through the row pass,
    rounding right shifts, output scaled by 8"""
    def one_pass(d, first):
        d = [d[..., i] for i in range(8)]
        t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        n = 11 if first else 15

        def ds(x, n=n):
            return (x + (1 << (n - 1))) >> n
        o = [None] * 8
        o[0], o[4] = ((t10 + t11) << 2, (t10 - t11) << 2) if first else (ds(t10 + t11, 2), ds(t10 - t11, 2))
        z1 = (t12 + t13) * 4433
        o[2], o[6] = ds(z1 + t13 * 6270), ds(z1 - t12 * 15137)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        o[7], o[5], o[3], o[1] = ds(t4 * 2446 + z1 + z3), ds(t5 * 16819 + z2 + z4), ds(t6 * 25172 + z2 + z3), ds(t7 * 12299 + z1 + z4)
        return np.stack(o, axis=-1)
    rows = one_pass(b, True)
    return np.swapaxes(one_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def model_coefficients(img, quality):
    """img uint8 [3, h, w] -> int16 [h/16 * w/16 * 6, 64]: colour, 2x2 chroma mean, level shift, DCT, quantisation; zigzag, scan order"""
    R, G, B = (img[i].astype(np.int64) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    h, w = Y.shape
    bias = np.tile(np.array([1, 2]), w // 4)[None, :]
    Cb, Cr = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2 for c in (Cb, Cr))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    ql, qc = (np.clip((np.array(base) * scale + 50) // 100, 1, 255).reshape(8, 8) * 8 for base in (BASE_LUMA, BASE_CHROMA))
    px, q8 = [], []
    for my in range(h // 16):
        for mx in range(w // 16):
            for by in range(2):
                for bx in range(2):
                    px.append(Y[my * 16 + by * 8:my * 16 + by * 8 + 8, mx * 16 + bx * 8:mx * 16 + bx * 8 + 8])
                    q8.append(ql)
            for c in (Cb, Cr):
                px.append(c[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8])
                q8.append(qc)
    c, q8 = model_fdct(np.stack(px) - 128), np.stack(q8)
    v = np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)
    return v.reshape(-1, 64)[:, ZIGZAG].astype(np.int16)
