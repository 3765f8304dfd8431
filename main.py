"""Unified CLI of the MI355X-native noise-trajectory-search path -- same flags as the reference's main.py:84-97.

    python main.py --backend edm --scorer imagenet --method eps_greedy --N 64 --K 4
    python main.py --backend edm --scorer brightness --method rejection --N 16 --network random:ddpmpp_cifar10

Arguments (verbatim from the reference):
    --backend   : 'sd' or 'edm' (required)
    --scorer    : 'brightness', 'compressibility', 'clip', or 'imagenet' (required)
    --method    : naive | rejection | beam | mcts | zero_order | eps_greedy (default naive)
    --prompt, --output, --N, --lambda_, --eps, --K, --B, --S, --seed, --device
Additions (the reference hard-codes a checkpoint URL, main.py:157-158; there is no network here):
    --network   : 'random:adm_imagenet64[:seed]' (default), 'random:ddpmpp_cifar10[:seed]', 'random:ncsnpp_cifar10[:seed]',
                  'random:ncsnpp_ffhq64[:seed]', 'random:vp_cifar10[:seed]', 'random:ve_cifar10[:seed]', 'random:iddpm_imagenet64[:seed]'
                  (the VP, VE and iDDPM preconditioners), the local path of an NVIDIA EDM network pickle (*.pkl, read without executing
                  its embedded source: EDMPrecond, VPPrecond, VEPrecond or iDDPMPrecond over the ADM, DDPM++ or NCSN++ U-Net, i.e. the
                  published edm-*.pkl and baseline-*.pkl files), or a .pt bundle.  sigma_min / sigma_max of the schedule (0.002, 80) are
                  clamped to the network's range, as the reference's edm/generate.py:31-32 does (the identity for EDMPrecond)
    --dtype     : f16x3 (default: split precision on the 16-bit matrix cores -- the reference's fp32 rewards and therefore its selected
                  candidates on the same seed, ~2.6x the f32 mode's speed) | f32 (parity mode, f32 matrix instruction) | bf16 | f16
                  (throughput modes: ~2.8x faster again, but a near-tied pick differs after ~10 decisions and the result is another sample)
                  | auto (f16 when the network pickle records use_fp16=True, f16x3 otherwise; the choice is printed)
    --unet      : SD backend: diffusers (default: the stock UNet2DConditionModel) | hip (sd_unet.SDUNet on this build's kernels, read from
                  $DTS_SD_UNET_DIR or the cached snapshot's unet/; no fallback).  --vae hip|diffusers likewise (default hip)
    --unet-head-dims: --unet hip: padded (default: head dims 40 / 80 / 160 zero-padded to 64 / 128 / 256 at load time) | native (as stored)
    --unet-downsample: --unet hip: s2d (default: the stride-2 downsamplers as space-to-depth + a stride-1 conv over 4C channels) | strided
              (the stride-2 3x3 convolution itself: a quarter of the multiply-adds, no space-to-depth pass); refused without --unet hip
    --text-encoder: SD backend: transformers (default: the stock CLIPTextModel) | hip (clip_text.CLIPTextTower on this build's kernels, read
                  from $DTS_SD_TEXT_ENCODER_DIR or the cached snapshot's text_encoder/; no fallback)
    --clip-tower: SD backend, --scorer clip: transformers (default: the stock CLIPModel image tower, float32 like the reference) | hip
                  (clip_vision.CLIPVisionTower on this build's kernels; no fallback).  --clip-tower-dtype f16 (default) | bf16: 16-bit
                  throughput modes of the scorer | f16x3: the parity-grade mode (float32 activations, split-precision matrix products)
    --clip-text-tower: SD backend, --scorer clip: transformers (default: the stock CLIPModel text tower, float32 like the reference) | hip
                  (clip_text.CLIPTextTower on this build's kernels; no fallback).  --clip-text-tower-dtype f16 | bf16 | f16x3 (default: follow
                  --clip-tower-dtype; f16x3 must be asked for here: clip_text.CLIPTextTowerX3, the parity-grade text tower).  Both towers at
                  the reference's precision: --clip-tower hip --clip-tower-dtype f16x3 --clip-text-tower hip --clip-text-tower-dtype f16x3
                  (--text-encoder hip, the SD text encoder, stays float16: the reference runs SD in float16)
    --jpeg-codec: --scorer compressibility: pil (default: the reference's host encode per image) | hip (the same byte count computed on the
                  GPU, identical rewards; image sides must be multiples of 16; no fallback)
    --beam      : EDM backend, --method beam: reference (default: the reference's branch as it stands -- it reads fields SamplingParams does not
                  define and raises AttributeError on entry) | run (the search that branch sets out to do: --B beams per image, the reference's
                  k, x --N candidates per beam, its b; per sigma step the top B of the B*N rewards survive, exact ties to the lower flat index;
                  generate_image_grid(beam_search=True)).  --backend sd has a working beam search of its own and ignores the flag
    --share-identical: EDM backend, --method eps_greedy | zero_order | beam (--beam run): at the sigma steps without churn noise (sigma
                  outside [S_min, S_max]: steps 0, 1, 15, 16 and 17 of the 18) all candidates of an image are the same row; evaluate it once
                  (generate_image_grid(share_identical=True)): same image and selections, fewer denoiser rows than the reference's count
    --seeds LIST --outdir DIR [--subdirs] [--class N]: bulk mode (flags of the reference's edm/generate.py): one search per
                  seed, <outdir>/<seed:06d>.png; with torch.distributed.run the SEEDS are split over the ranks (no collective)
    --search-batch S: bulk mode: the searches of S seeds run in lock-step as ONE batch (S x the rows per denoiser call; every image draws
                  from its own seed's stream, so a seed's search does not depend on its companions; default 1; --method mcts runs per seed
                  unless --mcts-lockstep is given)
                  --backend sd: the same flags (--seeds --outdir [--subdirs] [--search-batch S]); seed s draws what `--seed s` draws, --method
                  rejection runs its N naive trajectories as N rows per seed, and `--decode-rows R` caps the rows per VAE decode and scorer
                  call (at [n,3,512,512] the decoder needs it for large S x N)
    python main.py --backend sd --scorer clip --method eps_greedy --N 4 --K 2 --unet hip --seeds 0-63 --search-batch 8 --decode-rows 16 --outdir out
    --mcts-lockstep: EDM backend, bulk mode, --method mcts: the trees of the S seeds of a search batch advance as one batch, aligned by
                  simulation index (generate_image_grid(mcts_lockstep=True)); seed s draws its rollout children from
                  numpy.random.RandomState(s) instead of numpy's global generator
    python main.py --backend edm --scorer imagenet --method mcts --N 4 --S 16 --seeds 0-15 --search-batch 16 --mcts-lockstep --outdir out
Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N main.py ...`; the N candidates of every
search iteration are sharded across the ranks (diffusion_tts_amd/parallel.py).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


CLIP_TOWER_DTYPES = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f16x3': 'f16x3'}      # --clip-tower-dtype -> CLIPVisionTower dtype


def get_scorer(backend, scorer_name, device, compute_dtype=None, clip_tower='transformers', clip_model=None, jpeg_codec='pil',
               clip_tower_dtype='f16', clip_text_tower='transformers', clip_text_tower_dtype=None):
    """main.py:60-71 of the reference.  compute_dtype: the search's --dtype; the ImageNet classifier runs in the search's own mode for the two parity
    modes (float32, f16x3) and in float16 otherwise (also beside a bfloat16 denoiser: scorers.ImageNetScorer).  clip_tower: --clip-tower,
    clip_tower_dtype: --clip-tower-dtype (the activations of the 'hip' tower); clip_model: a transformers.CLIPModel to score with instead of the cached checkpoint (scorers.CLIPScorer model=).  jpeg_codec: --jpeg-codec.
    clip_text_tower: --clip-text-tower, clip_text_tower_dtype: --clip-text-tower-dtype (None: the text tower follows clip_tower_dtype)."""
    from diffusion_tts_amd import scorers as S
    if scorer_name == 'brightness':
        return S.BrightnessScorer(dtype=torch.float32)
    if scorer_name == 'compressibility':                               # sd/scorers.py:79 normalises by 150000 bytes, edm/scorers.py:177 by 3000
        return S.CompressibilityScorer(dtype=torch.float32, max_size=150000 if backend == 'sd' else 3000, codec=jpeg_codec)
    if scorer_name == 'imagenet' and backend == 'edm':
        return S.ImageNetScorer(dtype=torch.float32, device=device, compute_dtype=compute_dtype if compute_dtype in (torch.float32, 'f16x3') else torch.float16)
    if scorer_name == 'clip' and backend == 'sd':
        return S.CLIPScorer(dtype=torch.float32, device=device, model=clip_model, vision_tower=clip_tower,
                            tower_dtype=CLIP_TOWER_DTYPES[clip_tower_dtype], text_tower=clip_text_tower,
                            text_tower_dtype=None if clip_text_tower_dtype is None else CLIP_TOWER_DTYPES[clip_text_tower_dtype])
                            # (local HF cache only; raises with instructions otherwise)
    raise ValueError(f"Unknown or invalid scorer '{scorer_name}' for backend '{backend}'")


def load_sd_vae(model_id, dev, kind='hip'):
    """The SD VAE of the search loop.  kind='hip' (default): this build's HIP decoder (vae.VAEDecoder, drop-in for `vae.decode`) read from
    the safetensors `vae/` directory of the locally cached SD-1.5 snapshot (or $DTS_SD_VAE_DIR) -- and an error when that directory cannot
    be found or read: there is no silent fallback.  kind='diffusers' (`--vae diffusers`): the stock AutoencoderKL module, chosen explicitly."""
    if kind == 'diffusers':
        from diffusers import AutoencoderKL
        return AutoencoderKL.from_pretrained(model_id, subfolder='vae', torch_dtype=torch.float16, local_files_only=True).to(dev)
    if kind != 'hip':
        raise ValueError(f"--vae must be 'hip' or 'diffusers', got {kind!r}")
    from diffusion_tts_amd.vae import VAEDecoder
    path = os.environ.get('DTS_SD_VAE_DIR')
    if path is None:
        from huggingface_hub import snapshot_download
        path = os.path.join(snapshot_download(model_id, local_files_only=True, allow_patterns=['vae/*']), 'vae')
    if not os.path.isdir(path):
        raise FileNotFoundError(f'SD VAE directory {path!r} not found (set DTS_SD_VAE_DIR, or pass --vae diffusers for the stock module)')
    return VAEDecoder.from_pretrained(path, device=dev, dtype=torch.float16)


def load_sd_unet(model_id, dev, kind='diffusers', head_dims='padded', downsample='s2d'):
    """The SD U-Net of the search loop, the twin of load_sd_vae.  kind='hip' (`--unet hip`): this build's HIP U-Net (sd_unet.SDUNet, drop-in
    for `unet(sample, t, encoder_hidden_states=...)`) read from the safetensors `unet/` directory of the locally cached SD-1.5 snapshot (or
    $DTS_SD_UNET_DIR) -- and an error when that directory cannot be found or read: there is no silent fallback.  kind='diffusers' (the
    default): the stock UNet2DConditionModel module.  head_dims (`--unet-head-dims`, kind='hip' only): 'padded' (default) or 'native', see
    sd_unet.SDUNet; any other value is refused before a file is touched.  downsample (`--unet-downsample`): 's2d' (default) or 'strided',
    see sd_unet.SDUNet; any other value, and 'strided' with another kind than 'hip', is refused before a file is touched."""
    if head_dims not in ('padded', 'native'):
        raise ValueError(f"--unet-head-dims must be 'padded' or 'native', got {head_dims!r}")
    if downsample not in ('s2d', 'strided'):
        raise ValueError(f"--unet-downsample must be 's2d' or 'strided', got {downsample!r}")
    if downsample != 's2d' and kind != 'hip':
        raise ValueError(f"--unet-downsample {downsample} goes with --unet hip (the stock module has one downsampler), got --unet {kind}")
    if kind == 'diffusers':
        from diffusers import UNet2DConditionModel
        return UNet2DConditionModel.from_pretrained(model_id, subfolder='unet', torch_dtype=torch.float16, local_files_only=True).to(dev)
    if kind != 'hip':
        raise ValueError(f"--unet must be 'hip' or 'diffusers', got {kind!r}")
    from diffusion_tts_amd.sd_unet import SDUNet
    path = os.environ.get('DTS_SD_UNET_DIR')
    if path is None:
        from huggingface_hub import snapshot_download
        path = os.path.join(snapshot_download(model_id, local_files_only=True, allow_patterns=['unet/*']), 'unet')
    if not os.path.isdir(path):
        raise FileNotFoundError(f'SD U-Net directory {path!r} not found (set DTS_SD_UNET_DIR, or pass --unet diffusers for the stock module)')
    return SDUNet.from_pretrained(path, device=dev, dtype=torch.float16, head_dims=head_dims, downsample=downsample)


def load_sd_text_encoder(model_id, dev, kind='transformers'):
    """The SD text encoder, the twin of load_sd_unet.  kind='hip' (`--text-encoder hip`): this build's HIP text tower
    (clip_text.CLIPTextTower, drop-in for `text_encoder(input_ids, attention_mask=...)[0]`) read from the safetensors `text_encoder/`
    directory of the locally cached SD-1.5 snapshot (or $DTS_SD_TEXT_ENCODER_DIR) -- and an error when that directory cannot be found or
    read: there is no silent fallback.  kind='transformers' (the default): the stock CLIPTextModel module."""
    if kind == 'transformers':
        from transformers import CLIPTextModel
        return CLIPTextModel.from_pretrained(model_id, subfolder='text_encoder', torch_dtype=torch.float16, local_files_only=True).to(dev)
    if kind != 'hip':
        raise ValueError(f"--text-encoder must be 'hip' or 'transformers', got {kind!r}")
    from diffusion_tts_amd.clip_text import CLIPTextTower
    path = os.environ.get('DTS_SD_TEXT_ENCODER_DIR')
    if path is None:
        from huggingface_hub import snapshot_download
        path = os.path.join(snapshot_download(model_id, local_files_only=True, allow_patterns=['text_encoder/*']), 'text_encoder')
    if not os.path.isdir(path):
        raise FileNotFoundError(f'SD text encoder directory {path!r} not found (set DTS_SD_TEXT_ENCODER_DIR, or pass --text-encoder '
                                f'transformers for the stock module)')
    return CLIPTextTower.from_pretrained(path, device=dev, dtype=torch.float16)


def main_sd(args):
    """SD backend (reference main.py:111-147).  The search loop, the fused DDIM candidate step and candidate batching are
    this build's (diffusion_tts_amd/sd_pipeline.py), and so are the VAE decoder (`--vae hip`, the default) and, with `--unet hip`, the
    U-Net (diffusion_tts_amd/sd_unet.py) and, with `--text-encoder hip`, the text encoder (diffusion_tts_amd/clip_text.py):
    `--unet hip --vae hip --text-encoder hip` needs of transformers the tokenizer only (CLIPTokenizer: host string processing and
    vocabulary files) and SD-1.5 weights in the local HF cache.  `--unet diffusers` (the default) / `--vae diffusers` take the stock
    diffusers modules on PyTorch-ROCm, `--text-encoder transformers` (the default) the stock CLIPTextModel."""
    unet_kind, vae_kind = getattr(args, 'unet', 'diffusers'), getattr(args, 'vae', 'hip')
    te_kind = getattr(args, 'text_encoder', 'transformers')
    try:
        if 'diffusers' in (unet_kind, vae_kind):                           # only the parts that are asked for need diffusers
            import diffusers                                               # noqa: F401
        from transformers import CLIPTokenizer                             # (--text-encoder hip: nothing else of transformers)
    except Exception as e:      # pragma: no cover
        raise RuntimeError('--backend sd needs `transformers` (the tokenizer; with --text-encoder transformers also the text encoder) and, '
                           'for --unet diffusers / --vae diffusers, `diffusers`, with SD-1.5 weights in the local cache; that import '
                           'failed.  `--unet hip --vae hip --text-encoder hip` runs without diffusers and with the tokenizer alone; '
                           'or drive diffusion_tts_amd.sd_pipeline.SDSearchPipeline(unet, vae) directly (tests/test_gpu_sd_unet.py '
                           'shows the call).') from e
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    import torch.distributed as dist
    model_id = 'runwayml/stable-diffusion-v1-5'
    world, local = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:                                 # one process per GPU: the candidates of every search decision are sharded (sd_pipeline.py)
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    dev = torch.device('cuda', local) if world > 1 else torch.device(args.device)
    unet = load_sd_unet(model_id, dev, unet_kind, head_dims=getattr(args, 'unet_head_dims', 'padded'),
                        downsample=getattr(args, 'unet_downsample', 's2d'))
    vae = load_sd_vae(model_id, dev, vae_kind)
    tok = CLIPTokenizer.from_pretrained(model_id, subfolder='tokenizer', local_files_only=True)
    te = load_sd_text_encoder(model_id, dev, te_kind)

    scorer = get_scorer('sd', args.scorer, dev, clip_tower=getattr(args, 'clip_tower', 'transformers'),
                        jpeg_codec=getattr(args, 'jpeg_codec', 'pil'), clip_tower_dtype=getattr(args, 'clip_tower_dtype', 'f16'),
                        clip_text_tower=getattr(args, 'clip_text_tower', 'transformers'),
                        clip_text_tower_dtype=getattr(args, 'clip_text_tower_dtype', None))
    params = {'N': args.N, 'lambda': args.lambda_, 'eps': args.eps, 'K': args.K, 'B': args.B, 'S': args.S}
    if getattr(args, 'seeds', None) is not None:                               # bulk mode: the SEEDS are split over the ranks, whole searches per rank
        from diffusion_tts_amd.bulk import generate_sd_seeds
        from diffusion_tts_amd.parallel import CandidateShards
        pipe = SDSearchPipeline(unet, vae, device=dev, text_encoder=te, tokenizer=tok, shards=CandidateShards(enabled=False))
        done = generate_sd_seeds(pipe, args.prompt, args.seeds, args.outdir, method=args.method, params=params, search_batch=args.search_batch,
                                 num_inference_steps=50, score_function=scorer, subdirs=args.subdirs, decode_rows=args.decode_rows)
        print(f'[SD] rank {os.environ.get("RANK", "0")}: {len(done)} images -> {args.outdir}')
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return done
    pipe = SDSearchPipeline(unet, vae, device=dev, text_encoder=te, tokenizer=tok)     # encodes the prompt itself (pipeline...:976-992)
    torch.manual_seed(args.seed)                                                       # same host RNG stream on every rank
    best, best_score = None, float('-inf')
    for _ in range(params['N'] if args.method == 'rejection' else 1):          # reference main.py:134
        lat = torch.randn(1, unet.config.in_channels, unet.config.sample_size, unet.config.sample_size)
        out, score = pipe(prompt=args.prompt, latents=lat, num_inference_steps=50, score_function=scorer, method='naive' if args.method == 'rejection' else args.method,
                          params=params, output_type='pil')
        score = float(score.item() if torch.is_tensor(score) else score)
        if score > best_score:
            best, best_score = out, score
    outname = args.output or f'sd_{args.method}_{args.scorer}.png'
    if int(os.environ.get('RANK', '0')) == 0:
        best.images[0].save(outname)
        print(f'\n[SD] Saved: {outname}\nBest score: {best_score}  (U-Net: {type(unet).__name__}, VAE: {type(vae).__name__}, text encoder: {type(te).__name__}, reward collectives: {best.collectives})\n')
        if unet_kind == 'hip':
            print(f'[SD] U-Net forwards: {unet._graphs.path_report()}\n')
    if world > 1:
        dist.destroy_process_group()
    return best


class _Parser(argparse.ArgumentParser):
    """the flags that only go together are refused where the command line is parsed (usage message, exit status 2)"""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if getattr(ns, 'unet_downsample', 's2d') != 's2d' and getattr(ns, 'unet', 'diffusers') != 'hip':
            self.error(f'--unet-downsample {ns.unet_downsample} goes with --unet hip, got --unet {ns.unet}')
        return ns


def build_parser():
    parser = _Parser(description='Unified Diffusion Image Generator (EDM/SD), MI355X-native hot path',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument('--backend', type=str, choices=['edm', 'sd'], required=True, help='Backend: edm or sd')
    parser.add_argument('--scorer', type=str, choices=['brightness', 'compressibility', 'clip', 'imagenet'], required=True,
                        help='Scorer name')
    parser.add_argument('--method', type=str, default='naive',
                        help='Sampling method (naive, rejection, beam, mcts, zero_order, eps_greedy)')
    parser.add_argument('--prompt', type=str, default='YOUR PROMPT HERE', help='Prompt for SD')
    parser.add_argument('--output', type=str, default=None, help='Output filename (default: auto)')
    parser.add_argument('--N', type=int, default=4, help='Master param N')
    parser.add_argument('--lambda_', type=float, default=0.15, help='Master param lambda')
    parser.add_argument('--eps', type=float, default=0.4, help='Master param eps')
    parser.add_argument('--K', type=int, default=20, help='Master param K')
    parser.add_argument('--B', type=int, default=2, help='Master param B')
    parser.add_argument('--S', type=int, default=8, help='Master param S')
    parser.add_argument('--seed', type=int, default=0, help='Random seed')
    parser.add_argument('--device', type=str, default='cuda', help='Device')
    parser.add_argument('--network', type=str, default='random:adm_imagenet64', help='EDM network spec (see module docstring)')
    parser.add_argument('--dtype', type=str, default='f16x3', choices=['bf16', 'f16', 'f32', 'f16x3', 'auto'], help='compute mode (see the module docstring)')
    parser.add_argument('--vae', type=str, default='hip', choices=['hip', 'diffusers'],
                        help="SD backend: 'hip' = this build's VAE decoder (an error if its safetensors cannot be read), 'diffusers' = the stock module")
    parser.add_argument('--unet', type=str, default='diffusers', choices=['hip', 'diffusers'],
                        help="SD backend: 'hip' = this build's U-Net on the HIP kernels (an error if its safetensors cannot be read), 'diffusers' = the stock module")
    parser.add_argument('--unet-head-dims', dest='unet_head_dims', type=str, default='padded', choices=['padded', 'native'],
                        help="--unet hip: 'padded' = SD-1.x's head dims 40 / 80 / 160 zero-padded to 64 / 128 / 256 at load time, 'native' = kept as "
                             "stored (the attention kernels pad on chip; the q/k/v/out projections run at the model's own widths)")
    parser.add_argument('--unet-downsample', dest='unet_downsample', type=str, default='s2d', choices=['s2d', 'strided'],
                        help="--unet hip only: 's2d' = the three stride-2 downsamplers as space-to-depth + a stride-1 3x3 convolution over 4C channels, "
                             "'strided' = the stride-2 3x3 convolution itself (a quarter of the multiply-adds and of the packed weight)")
    parser.add_argument('--text-encoder', dest='text_encoder', type=str, default='transformers', choices=['transformers', 'hip'],
                        help="SD backend: 'hip' = this build's CLIP text tower on the HIP kernels in float16 (an error if its safetensors cannot be "
                             "read), 'transformers' = the stock CLIPTextModel")
    parser.add_argument('--clip-tower', dest='clip_tower', type=str, default='transformers', choices=['transformers', 'hip'],
                        help="SD backend, --scorer clip: 'hip' = the CLIP image tower on this build's kernels in float16 (a 16-bit throughput mode: the "
                             "reference scores in float32; an error if the kernels do not take the model's shape), 'transformers' = the stock module")
    parser.add_argument('--clip-tower-dtype', dest='clip_tower_dtype', type=str, default='f16', choices=['f16', 'bf16', 'f16x3'],
                        help="--clip-tower hip: the tower's activations.  f16 (default) / bf16: the 16-bit throughput modes; f16x3: the parity-grade "
                             "mode (float32 activations, split-precision matrix products: the float32 module's rewards to its own rounding error)")
    parser.add_argument('--clip-text-tower', dest='clip_text_tower', type=str, default='transformers', choices=['transformers', 'hip'],
                        help="SD backend, --scorer clip: 'hip' = the CLIP text tower on this build's kernels (an error if the kernels do not take the "
                             "model's shape), 'transformers' = the stock module, float32 like the reference")
    parser.add_argument('--clip-text-tower-dtype', dest='clip_text_tower_dtype', type=str, default=None, choices=['f16', 'bf16', 'f16x3'],
                        help="--clip-text-tower hip: the text tower's activations.  Default: follow --clip-tower-dtype (which selects a 16-bit text "
                             "tower only).  f16x3: the parity-grade text tower (float32 activations, split-precision matrix products, masked "
                             "split-precision attention)")
    parser.add_argument('--jpeg-codec', dest='jpeg_codec', type=str, default='pil', choices=['pil', 'hip'],
                        help="--scorer compressibility: 'hip' = the JPEG byte length computed on the GPU (identical rewards; image sides must be "
                             "multiples of 16, an error otherwise), 'pil' = the reference's host encode of every image")
    parser.add_argument('--beam', type=str, default='reference', choices=['reference', 'run'],
                        help="EDM backend, --method beam: 'reference' = the reference's branch as it stands (AttributeError on entry), 'run' = the "
                             "beam search it sets out to do: --B beams x --N candidates per beam (generate_image_grid(beam_search=True))")
    parser.add_argument('--share-identical', dest='share_identical', action='store_true',
                        help='EDM backend, eps_greedy / zero_order / beam (--beam run): evaluate the identical candidates of a sigma step without '
                             'churn noise once (generate_image_grid(share_identical=True)); same image, fewer denoiser rows')
    parser.add_argument('--seeds', type=str, default=None, help='bulk mode: seeds, e.g. 0-63 or 1,2,5-10 (one image per seed)')
    parser.add_argument('--outdir', type=str, default='out', help='bulk mode: output directory')
    parser.add_argument('--subdirs', action='store_true', help='bulk mode: one subdirectory per 1000 seeds')
    parser.add_argument('--search-batch', type=int, default=1,
                        help='bulk mode: run the searches of this many seeds in lock-step as one batch (default 1; mcts: one search per seed)')
    parser.add_argument('--mcts-lockstep', dest='mcts_lockstep', action='store_true',
                        help='EDM backend, bulk mode, --method mcts: run the MCTS searches of a search batch in lock-step as one batch '
                             '(generate_image_grid(mcts_lockstep=True)); without it mcts runs one search per seed')
    parser.add_argument('--decode-rows', dest='decode_rows', type=int, default=None,
                        help='SD backend, bulk mode: at most this many rows per VAE decode and scorer call (default: all rows of a batch at once)')
    parser.add_argument('--class', dest='class_idx', type=int, default=None, help='bulk mode: class label (default: per-seed random)')
    return parser


def check_bulk_args(args):
    """the bulk-mode flags that only go together: raised before anything is loaded"""
    if args.seeds is not None and args.search_batch < 1:
        raise ValueError(f'--search-batch: a positive number of seeds per lock-step batch, got {args.search_batch}')
    if getattr(args, 'mcts_lockstep', False):
        if args.backend != 'edm' or args.method != 'mcts':
            raise ValueError('--mcts-lockstep is an EDM option of --method mcts (the SD backend\'s MCTS runs one search per seed)')
        if args.seeds is None:
            raise ValueError('--mcts-lockstep goes with --seeds (bulk mode: the searches of a --search-batch run as one batch)')
    if args.decode_rows is not None:
        if args.backend != 'sd':
            raise ValueError('--decode-rows is an SD option (the rows per VAE decode of a lock-step batch)')
        if args.seeds is None:
            raise ValueError('--decode-rows goes with --seeds (the SD bulk mode)')
        if args.decode_rows < 1:
            raise ValueError(f'--decode-rows: a positive number of rows per VAE decode, got {args.decode_rows}')
    if args.backend == 'sd' and args.seeds is not None and args.output is not None:
        raise ValueError('--output names the one image of a single search; bulk mode (--seeds) writes <outdir>/<seed:06d>.png')


def main(argv=None):
    args = build_parser().parse_args(argv)

    if args.backend == 'sd' and args.scorer == 'imagenet':
        raise ValueError('imagenet scorer is only available for edm backend')
    if args.backend == 'edm' and args.scorer == 'clip':
        raise ValueError('clip scorer is only available for sd backend')
    check_bulk_args(args)
    if args.backend == 'sd':
        if getattr(args, 'share_identical', False):
            raise ValueError('--share-identical is an EDM option (DDIM with eta = 1 adds noise at every step)')
        if getattr(args, 'beam', 'reference') != 'reference':
            print(f'[SD] --beam {args.beam} is an EDM option: ignored (--method beam runs on the SD backend as it is)')
        return main_sd(args)
    if not str(args.device).startswith('cuda'):
        raise RuntimeError(f"--device {args.device}: this build is the GPU path; the CPU path is the reference itself "
                           f"(its restatement lives in oracle/ as test infrastructure)")

    import torch.distributed as dist
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    device = torch.device('cuda', local if world > 1 else (torch.device(args.device).index or 0))
    torch.cuda.set_device(device)

    from diffusion_tts_amd.sampler import SamplingMethod, generate_image_grid, load_network
    from diffusion_tts_amd.ops import F16X3
    dtype = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32, 'f16x3': F16X3, 'auto': 'auto'}[args.dtype]
    net = load_network(args.network, device=device, dtype=dtype)
    if args.dtype == 'auto':
        dtype = net.dtype
        args.dtype = 'f16' if dtype == torch.float16 else 'f16x3'
        print(f'[EDM] --dtype auto: {args.dtype} (the network records use_fp16={net.cfg.use_fp16})')
    scorer = get_scorer('edm', args.scorer, device, compute_dtype=dtype, jpeg_codec=getattr(args, 'jpeg_codec', 'pil'))
    # edm/generate.py:31-32: the schedule's end points inside the network's range (EDMPrecond: 0 .. inf, the identity).  Without it an iDDPM
    # network rounds 0.002 to u[M] = 0 and the last Heun step divides by t_hat = 0, as the reference's would
    sigma_min, sigma_max = max(0.002, net.sigma_min), min(80, net.sigma_max)
    beam_run = getattr(args, 'beam', 'reference') == 'run'
    if beam_run and args.method != 'beam':
        raise ValueError(f'--beam run goes with --method beam, got --method {args.method}')
    extras = dict(beam_search=True) if beam_run else {}
    if getattr(args, 'share_identical', False):
        extras['share_identical'] = True
    if getattr(args, 'mcts_lockstep', False):
        extras['mcts_lockstep'] = True
    if args.seeds is not None:                                                        # bulk mode: seeds sharded over the ranks
        from diffusion_tts_amd.bulk import generate_seeds
        mm = {'naive': SamplingMethod.NAIVE, 'rejection': SamplingMethod.REJECTION_SAMPLING, 'beam': SamplingMethod.BEAM_SEARCH,
              'mcts': SamplingMethod.MCTS, 'zero_order': SamplingMethod.ZERO_ORDER, 'eps_greedy': SamplingMethod.EPS_GREEDY}
        sp = {'scorer': scorer}
        if args.method != 'naive':
            sp.update(N=args.N, K=args.K, lambda_param=args.lambda_, eps=args.eps, B=args.B, S=args.S)
        done = generate_seeds(net, args.seeds, args.outdir, sampling_method=mm[args.method], sampling_params=sp,
                              class_idx=args.class_idx, subdirs=args.subdirs, device=device, compute_dtype=dtype, search_batch=args.search_batch,
                              num_steps=18, S_churn=40, S_min=0.05, S_max=50, S_noise=1.003, sigma_min=sigma_min, sigma_max=sigma_max, **extras)
        print(f'[EDM] rank {os.environ.get("RANK", "0")}: {len(done)} images -> {args.outdir}')
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return done
    num_images = 1
    r = net.img_resolution
    latents = torch.randn([num_images, net.img_channels, r, r])                       # drawn before seeding, as main.py:161
    class_labels = torch.eye(net.label_dim)[torch.randint(net.label_dim, size=[num_images])] if net.label_dim else None
    if world > 1:                                                                      # replicate the unseeded draws
        latents, class_labels = latents.to(device), None if class_labels is None else class_labels.to(device)
        dist.broadcast(latents, 0)
        if class_labels is not None:
            dist.broadcast(class_labels, 0)
        latents, class_labels = latents.cpu(), None if class_labels is None else class_labels.cpu()
    method_map = {'naive': SamplingMethod.NAIVE, 'rejection': SamplingMethod.REJECTION_SAMPLING,
                  'beam': SamplingMethod.BEAM_SEARCH, 'mcts': SamplingMethod.MCTS,
                  'zero_order': SamplingMethod.ZERO_ORDER, 'eps_greedy': SamplingMethod.EPS_GREEDY}
    if args.method not in method_map:
        raise ValueError(f'Unknown method: {args.method}')
    sampling_params = {'scorer': scorer}
    if args.method in ['rejection', 'zero_order', 'eps_greedy', 'beam', 'mcts']:
        sampling_params.update(N=args.N, K=args.K, lambda_param=args.lambda_, eps=args.eps, B=args.B, S=args.S)
    outname = args.output or f'edm_{args.method}_{args.scorer}.png'
    res = generate_image_grid(net, outname, latents, class_labels, seed=args.seed, gridw=1, gridh=1, device=device,
                              num_steps=18, sigma_min=sigma_min, sigma_max=sigma_max, S_churn=40, S_min=0.05, S_max=50, S_noise=1.003,
                              sampling_method=method_map[args.method], sampling_params=sampling_params, compute_dtype=dtype, **extras)
    if int(os.environ.get('RANK', '0')) == 0:
        print(f'\n[EDM] Saved: {outname}  (denoiser rows: {res["net_rows"]}, reward collectives: {res["collectives"]})')
        print(f'[EDM] compute mode {args.dtype}; denoiser forwards: {net._graphs.path_report()}\n')
    if world > 1:
        dist.destroy_process_group()
    return res


if __name__ == '__main__':
    main()
