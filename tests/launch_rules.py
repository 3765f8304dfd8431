"""Host launch rules restated in Python, and the cases that take the SECOND trip of the loops those rules size.

Several kernels contain a loop whose trip count the host launcher derives from the problem size; at the small shapes the references
like, every such loop runs once.  Nothing reports which form ran, so each rule is written out here a second time, from the launcher's
text, and the tables below say what each case must reach.  tests/test_launch_rules.py asserts the tables against the rules on the CPU (a
changed cap or heuristic in the library has to be restated here, and then fails there unless the shapes still pass it); the GPU files
assert the same per case and run the kernels.  (The convolutions' rules live with their cases in tests/conv_reference.py.)  Plain Python:
no torch, nothing of diffusion_tts_amd."""
import collections


def ceil_div(a, b):
    return -(-a // b)


# ---- dts_cross_attention (csrc/transformer.hip) -----------------------------------------------------------------------------------------
def xattn_plan(n, heads, tq):
    """(chunks of 64 queries, qchunks = chunks a block walks, qblocks = blocks per (sample, head)): qchunks doubles, up to 8, while
    n * heads * ceil(chunks / (2 * qchunks)) >= 1024 -- the staging of K / V is shared as widely as still leaves ~4 blocks per CU"""
    nh, chunks, qchunks = n * heads, ceil_div(tq, 64), 1
    while qchunks < 8 and nh * ceil_div(chunks, 2 * qchunks) >= 1024:
        qchunks *= 2
    return chunks, qchunks, ceil_div(chunks, qchunks)


XAttn = collections.namedtuple('XAttn', 'n heads d tq tk contexts chunks qchunks qblocks')
# every tq leaves a ragged last chunk (tq % 64 != 0) and a last block with chunks past the end (the wave-uniform `break`)
XATTN_CHUNK_LOOP = [
    XAttn(8, 16, 64, 1030, 77, None, 17, 2, 9),         # the last block holds chunk 16 alone: 6 queries, waves 1..3 break at once
    XAttn(8, 16, 64, 1800, 77, None, 29, 4, 8),         # the last block holds chunk 28 (8 queries) and three chunks past the end
    XAttn(64, 16, 64, 513, 128, None, 9, 8, 2),         # the second block holds chunk 8 (1 query) and seven chunks past the end
    XAttn(64, 16, 64, 581, 77, 2, 10, 8, 2),            # kv_rows over 2 contexts; chunks 8 and 9 (5 queries) in the second block
    XAttn(64, 2, 256, 1030, 77, None, 17, 2, 9),        # d = 256: 16 output tiles per chunk, 102 KiB of LDS at 77 (96 staged) keys
]


# ---- gn_apply_impl (csrc/groupnorm.hip) ----------------------------------------------------------------------------------------------------
GnApply = collections.namedtuple('GnApply', 'kernel k ppb blocks trips last_block_pixels threads w16')
GN_GRID_CAP = 4096          # blocks of 256 threads: grid_for()


def gn_apply_plan(n, c1, c2, h, w, f32, pool=False, split=False, gn_fuse=-1):
    """Which apply kernel serves a shape and how many trips its loop makes.
    rows (gn_apply_rows_kernel): unpooled, at most 256 16-byte chunks per pixel.  k = 256 // chunks pixels per block pass; a block owns ppb =
    ceil(n * hw / 4096) pixels of one sample, rounded up to a multiple of 2k; a thread walks its pixels two per trip (p and p + k, then
    p += 2k) and a single one at the end of a ragged last block.  trips = ppb / 2k, the pair trips of a thread in a whole block.  w16 (split
    image only): the 16-byte lane-pair store form, taken iff c1 % 8 == 0 and gn_fuse != 2.
    grid (gn_apply_kernel): every pooled apply and every wider row; one thread per chunk of an OUTPUT pixel, grid-stride over at most 4096
    blocks of 256.  trips = the most a thread makes."""
    c = c1 + c2
    chunks = c // (4 if f32 else 8)
    if pool or chunks > 256 or n > 65535:
        ho, wo = (h // 2, w // 2) if pool else (h, w)
        threads = n * ho * wo * chunks
        blocks = max(1, min(ceil_div(threads, 256), GN_GRID_CAP))
        return GnApply('grid', None, None, blocks, ceil_div(threads, 256 * blocks), None, threads, None)
    k, hw = 256 // chunks, h * w
    ppb = ceil_div(ceil_div(n * hw, 4096), 2 * k) * 2 * k
    bx = ceil_div(hw, ppb)
    return GnApply('rows', k, ppb, (bx, n), ppb // (2 * k), hw - (bx - 1) * ppb, None, bool(split and c1 % 8 == 0 and gn_fuse != 2))


GnCase = collections.namedtuple('GnCase', 'n c1 c2 h w dtypes pool expect')
# expect: the fields of GnApply the case must reach (the others are not pinned)
GN_ROWS_TWO_TRIPS = {
    # k = 1: 1024 blocks of 4 pixels per sample; the last has 3: one pair and the single-pixel tail
    'c1024': GnCase(3, 1024, 0, 65, 63, ('f32',), False, dict(kernel='rows', k=1, ppb=4, trips=2, last_block_pixels=3)),
    # k = 3: 1036 whole blocks of 12 pixels
    'c576': GnCase(2, 576, 0, 112, 111, ('bf16', 'f16'), False, dict(kernel='rows', k=3, ppb=12, trips=2, last_block_pixels=12)),
    # k = 5: 418 blocks of 20 pixels and one of 12: a pair for every pixel row, then the tail for rows 0 and 1
    'c192': GnCase(5, 192, 0, 92, 91, ('f32',), False, dict(kernel='rows', k=5, ppb=20, trips=2, last_block_pixels=12)),
    # the same tensor as a concat whose first half is no multiple of 8 channels: the split image's 8-byte store form whatever the knob says
    'c100+92': GnCase(5, 100, 92, 92, 91, ('f32',), False, dict(kernel='rows', k=5, ppb=20, trips=2, last_block_pixels=12)),
}
GN_GRID_TWO_TRIPS = {
    # 4096 * 256 = 1,048,576 threads per trip
    'pool_f32': GnCase(2, 192, 0, 50, 874, ('f32',), True, dict(kernel='grid', blocks=4096, trips=2, threads=1048800)),         # + 224
    'pool_16bit': GnCase(4, 192, 0, 50, 874, ('bf16', 'f16'), True, dict(kernel='grid', blocks=4096, trips=2, threads=1048800)),   # + 224
    'wide_f32': GnCase(1, 1536, 0, 1, 2731, ('f32',), False, dict(kernel='grid', blocks=4096, trips=2, threads=1048704)),       # + 128
}


# ---- dts_layer_norm / dts_vit_head (csrc/transformer.hip, csrc/vit.hip) ---------------------------------------------------------------------
def layer_norm_vectors(c):
    """register vectors (8 channels per lane, 64 lanes) of a row: which of the four `i` iterations of the 16-bit kernels hold data, and how
    many lanes of the last one"""
    nvec = c // 8
    return ceil_div(nvec, 64), nvec - 64 * (ceil_div(nvec, 64) - 1)


# c -> (register vectors in use, lanes of the last one): 8 is the single-lane row, 1544 the fourth vector on ONE lane, 2048 all four whole
LAYER_NORM_WIDTHS = {8: (1, 1), 1544: (4, 1), 2048: (4, 64)}


# ---- dts_jpeg_size (csrc/jpeg.hip) ------------------------------------------------------------------------------------------------------------
JPEG_BLOCK_BUF_BYTES = 256          # bit-buffer bytes per 8x8 block (kBlockBufBytes)
JPEG_BLOCK_MAX_BITS = 64 * (16 + 11)     # the most a block costs: 64 coefficients of a 16-bit code and 11 value bits (kBlockMaxBits)
JpegLayout = collections.namedtuple('JpegLayout', 'nb coef bitoff totals bitbuf bytes')


def align256(x):
    return (x + 255) & ~255


def jpeg_layout(n, h, w):
    """byte offsets of the workspace's four arrays (layout() of the host part): int16 coefficients [n][nb][64], int bit counts / offsets
    [n][nb], int totals [n], the bit buffer of 256 bytes per block; every array starts on a multiple of 256 bytes"""
    nb = (h // 16) * (w // 16) * 6
    blocks = n * nb
    coef = 0
    bitoff = coef + align256(blocks * 128)
    totals = bitoff + align256(blocks * 4)
    bitbuf = totals + align256(n * 4)
    return JpegLayout(nb, coef, bitoff, totals, bitbuf, bitbuf + align256(blocks * JPEG_BLOCK_BUF_BYTES))


def jpeg_shape_ok(n, h, w):
    """shape_ok() of the host part: whole MCUs, the caps on n, h, w and on all blocks of a call, and the bits of one image's scan -- at the
    most a block can cost -- below 2^31, because bit counts, offsets and positions are int"""
    mcus = (h // 16) * (w // 16)
    return (1 <= n <= 65535 and h >= 16 and w >= 16 and h % 16 == 0 and w % 16 == 0 and h <= 16384 and w <= 16384
            and n * mcus * 6 <= 1 << 24 and mcus * 6 * JPEG_BLOCK_MAX_BITS < 1 << 31)


def jpeg_scan_plan(nb):
    """jpeg_scan_kernel, one workgroup of 256 threads per image: (per = blocks a thread sums and rewrites, busy = threads that own at least
    one block, last = blocks of the last busy thread); thread t owns [min(t * per, nb), min(t * per + per, nb))"""
    per = ceil_div(nb, 256)
    busy = ceil_div(nb, per)
    return per, busy, nb - (busy - 1) * per


# (h, w) -> (nb, per, busy, last) of every shape the stream tests run: one block per thread with idle threads (nb <= 256), 2 and 3 per
# thread with the upper threads clamped to nothing, 4 per thread with a last busy thread that owns 2 (the only clamp of `hi`: nb is a
# multiple of 6, so per = 2 and 3 divide it), and 24 per thread with every thread busy
JPEG_SCAN_SHAPES = {
    (16, 16): (6, 1, 6, 1),
    (32, 32): (24, 1, 24, 1),
    (64, 64): (96, 1, 96, 1),
    (48, 80): (90, 1, 90, 1),
    (80, 48): (90, 1, 90, 1),
    (112, 112): (294, 2, 147, 2),
    (176, 160): (660, 3, 220, 3),
    (48, 688): (774, 4, 194, 2),
    (512, 512): (6144, 24, 256, 24),
}
# (n, h, w) of every call of the stream tests
JPEG_STREAM_CALLS = [(9, 16, 16), (9, 48, 80), (9, 80, 48), (9, 112, 112), (9, 176, 160), (9, 48, 688), (1, 512, 512), (9, 32, 32),
                     (1, 64, 64), (5, 64, 64), (64, 64, 64)]


# ---- batches past 2^31 / 2^32 bytes per tensor (tests/large_rows.py, tests/test_gpu_large_rows.py) -------------------------------------------
# Every case of tests/test_gpu_large_rows.py: a batch of n rows made of 7 distinct samples (large_rows.row_map), ONE launch.  Per tensor: the
# shape of one sample, the element size, the bytes of the whole tensor, and which boundaries lie inside it -- '31': byte offset 2^31, '32':
# byte offset 2^32, 'e31': element index 2^31 (the last two coincide for 16-bit types).  Written out as numbers; tests/test_large_rows_cpu.py
# recomputes every one of them, holds the seeded map to the samples that straddle the boundaries and asks dts_conv_plan for the route of every
# dts_conv2d case (`plan`: the fields that must come back, besides splits == 1).
LargeTensor = collections.namedtuple('LargeTensor', 'name sample_shape itemsize bytes crosses')
LargeCase = collections.namedtuple('LargeCase', 'name family n tensors spec')
LARGE_CASES = collections.OrderedDict()


def _large(name, family, n, tensors, spec):
    assert name not in LARGE_CASES
    LARGE_CASES[name] = LargeCase(name, family, n, tuple(LargeTensor(t[0], t[1], t[2], t[3], tuple(t[4].split())) for t in tensors), spec)


_large('igemm_1x1_bf16', 'conv2d', 131079, [
    ('x', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('bias_nc', (64,), 2, 16778112, ''),
], {'mode': 'bf16', 'h': 16, 'w': 16, 'c1': 64, 'cout': 64, 'k': 1, 'up': 0, 'ep': 'bn', 'stats': False, 'gn': False, 'plan': {'kernel': 0, 'tile': 64}})
_large('igemm_3x3_f16', 'conv2d', 131079, [
    ('x', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('residual', (16, 16, 64), 2, 4295196672, '31 32 e31'),
], {'mode': 'f16', 'h': 16, 'w': 16, 'c1': 64, 'cout': 64, 'k': 3, 'up': 0, 'ep': 'br', 'stats': False, 'gn': False, 'plan': {'kernel': 0, 'tile': 64}})
_large('pp192_bf16', 'conv2d', 65535, [
    ('x', (16, 16, 64), 2, 2147450880, ''),
    ('out', (16, 16, 192), 2, 6442352640, '31 32 e31'),
], {'mode': 'bf16', 'h': 16, 'w': 16, 'c1': 64, 'cout': 192, 'k': 3, 'up': 0, 'ep': 'b', 'stats': False, 'gn': False, 'plan': {'kernel': 6}})
_large('pp192_res_stats_f16', 'conv2d', 65535, [
    ('x', (16, 16, 64), 2, 2147450880, ''),
    ('out', (16, 16, 192), 2, 6442352640, '31 32 e31'),
    ('residual', (16, 16, 192), 2, 6442352640, '31 32 e31'),
    ('stats', (4, 192, 2), 4, 402647040, ''),
], {'mode': 'f16', 'h': 16, 'w': 16, 'c1': 64, 'cout': 192, 'k': 3, 'up': 0, 'ep': 'br', 'stats': True, 'gn': False, 'plan': {'kernel': 6, 'stats_in_kernel': 1}})
_large('pp192_gn_bf16', 'conv2d', 65535, [
    ('x', (16, 16, 64), 2, 2147450880, ''),
    ('out', (16, 16, 192), 2, 6442352640, '31 32 e31'),
    ('gn_coef', (64, 2), 4, 33553920, ''),
], {'mode': 'bf16', 'h': 16, 'w': 16, 'c1': 64, 'cout': 192, 'k': 3, 'up': 0, 'ep': 'b', 'stats': False, 'gn': True, 'plan': {'kernel': 6, 'gn': 1}})
_large('x3_3x3', 'conv2d', 131079, [
    ('x', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('out', (16, 16, 64), 4, 8590393344, '31 32 e31'),
], {'mode': 'f16x3', 'h': 16, 'w': 16, 'c1': 32, 'cout': 64, 'k': 3, 'up': 0, 'ep': 'b', 'stats': False, 'gn': False, 'plan': {'kernel': 0, 'tile': 64}})
_large('f32_3x3', 'conv2d', 131079, [
    ('x', (16, 16, 32), 4, 4295196672, '31 32'),
    ('out', (16, 16, 64), 4, 8590393344, '31 32 e31'),
], {'mode': 'f32', 'h': 16, 'w': 16, 'c1': 32, 'cout': 64, 'k': 3, 'up': 0, 'ep': 'b', 'stats': False, 'gn': False, 'plan': {'kernel': 0, 'tile': 64}})
_large('up1_bf16', 'conv2d', 131079, [
    ('x', (8, 8, 128), 2, 2147598336, '31'),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
], {'mode': 'bf16', 'h': 8, 'w': 8, 'c1': 128, 'cout': 64, 'k': 3, 'up': 1, 'ep': 'b', 'stats': False, 'gn': False, 'plan': {'kernel': 0, 'tile': 64}})
_large('stride2_f16', 'conv2d', 131079, [
    ('x', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('out', (8, 8, 256), 2, 4295196672, '31 32 e31'),
], {'mode': 'f16', 'h': 16, 'w': 16, 'c1': 64, 'cout': 256, 'k': 3, 'up': -1, 'ep': 'b', 'stats': False, 'gn': False, 'plan': {'kernel': 0, 'tile': 128}})
_large('in3_mfma_bf16', 'conv_in3', 131079, [
    ('x', (3, 16, 16), 4, 402674688, ''),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
], {'mode': 'bf16', 'h': 16, 'w': 16, 'cout': 64, 'route': 'in3_mfma'})
_large('in3_direct_f16', 'conv_in3', 139818, [
    ('x', (3, 12, 20), 4, 402675840, ''),
    ('out', (12, 20, 64), 2, 4295208960, '31 32 e31'),
], {'mode': 'f16', 'h': 12, 'w': 20, 'cout': 64, 'route': 'in3_direct'})
_large('out3_tiled_bf16', 'conv_out3', 131079, [
    ('x', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('out', (3, 16, 16), 4, 402674688, ''),
], {'mode': 'bf16', 'h': 16, 'w': 16, 'c': 64, 'route': 'out3_tiled'})
_large('out3_direct_f16', 'conv_out3', 139818, [
    ('x', (12, 20, 64), 2, 4295208960, '31 32 e31'),
    ('out', (3, 12, 20), 4, 402675840, ''),
], {'mode': 'f16', 'h': 12, 'w': 20, 'c': 64, 'route': 'out3_direct'})
_large('gn_bf16_c192', 'groupnorm', 43698, [
    ('x', (16, 16, 192), 2, 4295688192, '31 32 e31'),
    ('out', (16, 16, 192), 2, 4295688192, '31 32 e31'),
    ('out_pool', (8, 8, 192), 2, 1073922048, ''),
    ('scale_shift', (384,), 2, 33560064, ''),
], {'mode': 'bf16', 'c': 192, 'h': 16, 'w': 16, 'routes': ('split', 'fused', 'strips'), 'apply': 'rows'})
_large('gn_f32_c192', 'groupnorm', 21853, [
    ('x', (16, 16, 192), 4, 4296474624, '31 32'),
    ('out', (16, 16, 192), 4, 4296474624, '31 32'),
    ('out_split', (16, 16, 384), 2, 4296474624, '31 32 e31'),
    ('out_pool', (8, 8, 192), 4, 1074118656, ''),
    ('scale_shift', (384,), 4, 33566208, ''),
], {'mode': 'f32', 'c': 192, 'h': 16, 'w': 16, 'routes': ('split', 'fused', 'strips'), 'apply': 'rows'})
_large('att16_d64_bf16', 'attention', 119845, [
    ('qkv', (70, 384), 2, 6442867200, '31 32 e31'),
    ('out', (70, 128), 2, 2147622400, '31'),
], {'form': '64/QT1', 'mode': 'bf16', 't': 70, 'heads': 2, 'd': 64})
_large('att_mask_d64_f16', 'attention', 119845, [
    ('qkv', (70, 384), 2, 6442867200, '31 32 e31'),
    ('out', (70, 128), 2, 2147622400, '31'),
], {'form': '64/MASK', 'mode': 'f16', 't': 70, 'heads': 2, 'd': 64})
_large('att_x3_d64', 'attention', 59926, [
    ('qkv_image', (70, 768), 2, 6443243520, '31 32 e31'),
    ('out', (70, 128), 4, 2147747840, '31'),
], {'form': 'x3/QT1', 'mode': 'f32', 't': 70, 'heads': 2, 'd': 64})
_large('att16_d40_bf16', 'attention', 191747, [
    ('qkv', (70, 240), 2, 6442699200, '31 32 e31'),
    ('out', (70, 80), 2, 2147566400, '31'),
], {'form': 'native/40', 'mode': 'bf16', 't': 70, 'heads': 2, 'd': 40})
_large('xattn_f16_kv_rows', 'rows', 239682, [
    ('q', (70, 128), 2, 4295101440, '31 32 e31'),
    ('out', (70, 128), 2, 4295101440, '31 32 e31'),
    ('kv_rows', (1,), 4, 958728, ''),
], {'op': 'xattn_f16_kv_rows', 'mode': 'f16', 'tq': 70, 'tk': 77, 'heads': 2, 'd': 64, 'contexts': 2})
_large('layer_norm_bf16', 'rows', 131079, [
    ('x', (8, 2048), 2, 4295196672, '31 32 e31'),
    ('out', (8, 2048), 2, 4295196672, '31 32 e31'),
], {'op': 'layer_norm_bf16', 'mode': 'bf16'})
_large('geglu_f16', 'rows', 262151, [
    ('x', (4, 4096), 2, 8590163968, '31 32 e31'),
    ('out', (4, 2048), 2, 4295081984, '31 32 e31'),
], {'op': 'geglu_f16', 'mode': 'f16'})
_large('cast_from_f32_bf16', 'rows', 131079, [
    ('x', (16384,), 4, 8590393344, '31 32 e31'),
    ('out', (16384,), 2, 4295196672, '31 32 e31'),
], {'op': 'cast_from_f32_bf16', 'mode': 'bf16'})
_large('cast_to_f32_f16', 'rows', 131079, [
    ('x', (16384,), 2, 4295196672, '31 32 e31'),
    ('out', (16384,), 4, 8590393344, '31 32 e31'),
], {'op': 'cast_to_f32_f16', 'mode': 'f16'})
_large('quantize_u8_f32', 'rows', 174770, [
    ('x', (3, 64, 64), 4, 8590295040, '31 32 e31'),
    ('out', (3, 64, 64), 1, 2147573760, '31 e31'),
], {'op': 'quantize_u8_f32'})
_large('u8_to_unit_f32', 'rows', 174770, [
    ('img', (3, 64, 64), 1, 2147573760, '31 e31'),
    ('out', (3, 64, 64), 4, 8590295040, '31 32 e31'),
], {'op': 'u8_to_unit_f32'})
_large('brightness', 'rows', 349533, [
    ('img', (3, 64, 64), 1, 4295061504, '31 32 e31'),
    ('out', (1,), 4, 1398132, ''),
], {'op': 'brightness'})
_large('cfg_combine_bf16', 'rows', 131079, [
    ('uncond', (16384,), 2, 4295196672, '31 32 e31'),
    ('cond', (16384,), 2, 4295196672, '31 32 e31'),
    ('out', (16384,), 2, 4295196672, '31 32 e31'),
], {'op': 'cfg_combine_bf16', 'mode': 'bf16'})
_large('nchw_to_nhwc_bf16', 'rows', 131079, [
    ('x', (64, 16, 16), 4, 8590393344, '31 32 e31'),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
], {'op': 'nchw_to_nhwc_bf16', 'mode': 'bf16'})
_large('nchw_to_nhwc_pad_f16', 'rows', 32775, [
    ('x', (4, 32, 32), 4, 536985600, ''),
    ('out', (32, 32, 64), 2, 4295884800, '31 32 e31'),
], {'op': 'nchw_to_nhwc_pad_f16', 'mode': 'f16'})
_large('nhwc_to_nchw_bf16', 'rows', 131079, [
    ('x', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('out', (64, 16, 16), 4, 8590393344, '31 32 e31'),
], {'op': 'nhwc_to_nchw_bf16', 'mode': 'bf16'})
_large('split3_f16', 'rows', 131079, [
    ('x', (16, 16, 32), 4, 4295196672, '31 32'),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
], {'op': 'split3_f16'})
_large('split2_f16', 'rows', 131079, [
    ('x', (16, 16, 32), 4, 4295196672, '31 32'),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
], {'op': 'split2_f16'})
_large('resample2x_up_bf16', 'rows', 131079, [
    ('x', (8, 8, 64), 2, 1073799168, ''),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
], {'op': 'resample2x_up_bf16', 'mode': 'bf16'})
_large('resample2x_down_f16', 'rows', 131079, [
    ('x', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('out', (8, 8, 64), 2, 1073799168, ''),
], {'op': 'resample2x_down_f16', 'mode': 'f16'})
_large('resample_fir_up_f16', 'rows', 131079, [
    ('x', (8, 8, 64), 2, 1073799168, ''),
    ('out', (16, 16, 64), 2, 4295196672, '31 32 e31'),
], {'op': 'resample_fir_up_f16', 'mode': 'f16'})
_large('resample_fir_down_bf16', 'rows', 131079, [
    ('x', (16, 16, 64), 2, 4295196672, '31 32 e31'),
    ('out', (8, 8, 64), 2, 1073799168, ''),
], {'op': 'resample_fir_down_bf16', 'mode': 'bf16'})
_large('edm_precond_in', 'rows', 174770, [
    ('x', (3072,), 8, 4295147520, '31 32'),
    ('sigma', (1,), 8, 1398160, ''),
    ('xin', (3072,), 4, 2147573760, '31'),
    ('coef', (4,), 4, 2796320, ''),
], {'op': 'edm_precond_in'})
_large('edm_precond_out', 'rows', 174770, [
    ('x', (3072,), 8, 4295147520, '31 32'),
    ('F', (3072,), 4, 2147573760, '31'),
    ('coef', (4,), 4, 2796320, ''),
    ('D', (3072,), 4, 2147573760, '31'),
], {'op': 'edm_precond_out'})
_large('heun_xhat_rows', 'rows', 174770, [
    ('x_cur', (3072,), 8, 4295147520, '31 32'),
    ('eps', (3072,), 4, 2147573760, '31'),
    ('noise_coef', (1,), 8, 1398160, ''),
    ('x_hat', (3072,), 8, 4295147520, '31 32'),
], {'op': 'heun_xhat_rows'})
_large('heun_euler_rows', 'rows', 174770, [
    ('x_hat', (3072,), 8, 4295147520, '31 32'),
    ('D', (3072,), 4, 2147573760, '31'),
    ('d_cur', (3072,), 8, 4295147520, '31 32'),
    ('x_next', (3072,), 8, 4295147520, '31 32'),
], {'op': 'heun_euler_rows'})
_large('heun_correct_rows', 'rows', 174770, [
    ('x_hat', (3072,), 8, 4295147520, '31 32'),
    ('D2', (3072,), 4, 2147573760, '31'),
    ('d_cur', (3072,), 8, 4295147520, '31 32'),
    ('x_next', (3072,), 8, 4295147520, '31 32'),
], {'op': 'heun_correct_rows'})
_large('candidate_noise_rows', 'rows', 174770, [
    ('pivot', (3072,), 8, 4295147520, '31 32'),
    ('g', (3072,), 8, 4295147520, '31 32'),
    ('out', (3072,), 8, 4295147520, '31 32'),
], {'op': 'candidate_noise_rows'})

_large('up2_phase_x3', 'conv2d', 32775, [
    ('x', (8, 8, 64), 2, 268492800, ''),
    ('out', (16, 16, 128), 4, 4295884800, '31 32'),
    ('residual', (16, 16, 128), 4, 4295884800, '31 32'),
], {'mode': 'f16x3', 'h': 8, 'w': 8, 'c1': 32, 'cout': 128, 'k': 3, 'up': 2, 'ep': 'br', 'stats': False, 'gn': False, 'plan': {'kernel': 0, 'tile': 128, 'phases': 1}})
_large('gelu_erf_bf16', 'rows', 131079, [
    ('x', (16384,), 2, 4295196672, '31 32 e31'),
    ('out', (16384,), 2, 4295196672, '31 32 e31'),
], {'op': 'gelu_erf_bf16', 'mode': 'bf16', 'kind': 'gelu'})
_large('quick_gelu_f16', 'rows', 131079, [
    ('x', (16384,), 2, 4295196672, '31 32 e31'),
    ('out', (16384,), 2, 4295196672, '31 32 e31'),
], {'op': 'quick_gelu_f16', 'mode': 'f16', 'kind': 'quick_gelu'})
_large('ddim_candidates_groups_bf16', 'rows', 65543, [
    ('x', (16384,), 2, 2147713024, '31'),
    ('e', (16384,), 2, 2147713024, '31'),
    ('z', (2, 16384), 2, 4295426048, '31 32 e31'),
    ('prev', (2, 16384), 2, 4295426048, '31 32 e31'),
    ('x0', (16384,), 2, 2147713024, '31'),
], {'op': 'ddim_candidates_groups_bf16', 'mode': 'bf16', 'ncand': 2})
_large('ddim_candidates_f16', 'rows', 131079, [
    ('x', (16384,), 2, 4295196672, '31 32 e31'),
    ('e', (16384,), 2, 4295196672, '31 32 e31'),
    ('prev', (16384,), 2, 4295196672, '31 32 e31'),
], {'op': 'ddim_candidates_f16', 'mode': 'f16'})
_large('candidate_noise_sd_rows_f16', 'rows', 131079, [
    ('pivot', (4, 64, 64), 2, 4295196672, '31 32 e31'),
    ('u', (4, 64, 64), 2, 4295196672, '31 32 e31'),
    ('out', (4, 64, 64), 2, 4295196672, '31 32 e31'),
    ('mode', (1,), 4, 524316, ''),
    ('scale', (3,), 4, 1572948, ''),
], {'op': 'candidate_noise_sd_rows_f16', 'mode': 'f16'})
_large('candidate_noise_sd_f16', 'rows', 131079, [
    ('u', (4, 64, 64), 2, 4295196672, '31 32 e31'),
    ('out', (4, 64, 64), 2, 4295196672, '31 32 e31'),
    ('mode', (1,), 4, 524316, ''),
    ('scale', (3,), 4, 1572948, ''),
], {'op': 'candidate_noise_sd_f16', 'mode': 'f16'})
_large('jpeg_size_cap', 'rows', 43690, [
    ('img', (3, 128, 128), 1, 2147450880, ''),
    ('sizes', (1,), 4, 174760, ''),
    ('ws_coef', (384, 64), 2, 2147450880, ''),
    ('ws_bitbuf', (384, 256), 1, 4294901760, '31 e31'),
], {'op': 'jpeg_size_cap', 'h': 128, 'w': 128, 'cap_blocks': 16777216})
_large('group_rows_cap', 'rows', 1024, [
    ('rows', (1055796,), 4, 4324540416, '31 32'),
    ('slot', (1,), 4, 4096, ''),
], {'op': 'group_rows_cap', 'cap_rows': 1024})


# The switch of dts_conv2d at the 32-bit limits, from both sides (64 -> 192 channels, 3x3, 16x16 samples, bf16): the ping-pong kernel's
# buffer descriptors carry 32-bit byte counts, so conv_pp_eligible hands the layer to the implicit GEMM once an operand reaches 2^31 bytes
# (n = 65535: the input is 32 KiB short of it), and conv_plan refuses 2^30 pixels (n = 2^22 samples of 256).
LARGE_CONV_SWITCH = dict(c1=64, cout=192, k=3, h=16, w=16, mode='bf16', last_pp=(65535, 6), first_igemm=(65536, 0),
                         last_accepted=(1 << 22) - 1, first_refused=1 << 22, refusal='too many pixels')
