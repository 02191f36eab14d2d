"""VAE above 512 x 512 (more than 4096 latent pixels): the mid-block attention as ONE rcdm_flash_attn launch (head dim 512,
csrc/attn_wide.hip) instead of the score-buffer form, against oracle/vae_oracle.py with the weights and the bounds of
tests/test_vae.py; and RCDMsPipeline at 512 x 576 with the HIP VAE."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import vae_oracle as V
from rcdms_amd import synth, vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(c):
    d = dict(c)
    d["norm_num_groups"] = d.pop("groups")
    return d


def _err(got, want):
    rel = float(((got - want) ** 2).mean().sqrt() / (want ** 2).mean().sqrt())
    mx = float((got - want).abs().max() / want.abs().max())
    return rel, mx


# ---------------------------------------------------------------------------------------------- CPU: the decision
def test_mid_attention_form_default():
    f = vae.mid_attention_form
    assert f(4096, 512, "auto") == "scores"          # every size that ran before keeps its launches
    assert f(1024, 512, "auto") == "scores" and f(64, 64, "auto") == "scores"
    assert f(4104, 512, "auto") == "flash"
    assert f(6144, 64, "auto") == "flash"            # narrow heads: the kernels that existed already
    assert f(16384, 512, "auto") == "flash" and f(6144, 256, "auto") == "flash"
    with pytest.raises(NotImplementedError, match="512"):
        f(6144, 1024, "auto")
    with pytest.raises(NotImplementedError):
        f(6144, 200, "auto")                         # above 160 only multiples of 64
    with pytest.raises(NotImplementedError, match="4096"):
        f(4092, 512, "auto")                         # the score-buffer form still wants hw % 8 == 0


def test_mid_attention_form_follows_the_switch():
    f = vae.mid_attention_form
    assert f(4096, 512, "1") == "flash" and f(64, 64, "1") == "flash" and f(4092, 512, "1") == "flash"
    assert f(4096, 512, "0") == "scores"
    with pytest.raises(NotImplementedError, match="rcdm_softmax_rows holds rows of <= 4096"):
        f(6144, 512, "0")                            # the behaviour before the flash form existed
    with pytest.raises(NotImplementedError):
        f(1024, 1024, "1")
    # the process's own setting is the default argument, read from the environment at import, and listed in TABLE
    code = ("from rcdms_amd import switches, vae; "
            "print(switches.VAE_FLASH, switches.TABLE['RCDM_VAE_FLASH'], vae.mid_attention_form(1024, 512))")
    for val, want in (("1", "1 1 flash"), ("0", "0 0 scores"), (None, "auto auto scores"), ("auto", "auto auto scores")):
        env = {k: v for k, v in os.environ.items() if k != "RCDM_VAE_FLASH"}
        if val is not None:
            env["RCDM_VAE_FLASH"] = val
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.split("\n")[0].strip() == want, (val, out.stdout, out.stderr)


# ---------------------------------------------------------------------------------------------- GPU: against the oracle
def _decoder(cfg, seed=31):
    m = vae.AutoencoderKLDecoder(**_cfg(cfg)).eval()
    sd = synth.procedural_state_dict(V.decoder_shapes(cfg), seed)
    m.load_state_dict(sd)
    return m.to("cuda"), sd


@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg,n,h,w", [("sd15", V.SD15_VAE, 1, 64, 96), ("tiny", V.tiny_vae_config(), 2, 96, 96)])
def test_hip_vae_decode_highres_vs_oracle(hiplib, name, cfg, n, h, w):
    """6144 (rectangular) and 9216 latent pixels: NotImplementedError before the flash form."""
    m, sd = _decoder(cfg)
    z = synth.normal_tensor(f"vae.{name}.z_hi", (n, 4, h, w), 32)
    got = m.decode(z.cuda()).sample.float().cpu()
    assert any(t.startswith("flash_attn ") for t in m._programs[(n, h, w)][1].plan.tags)
    assert not any(t.startswith("softmax_rows") for t in m._programs[(n, h, w)][1].plan.tags)
    with torch.no_grad():
        want = V.vae_decode(sd, cfg, z)
    assert got.shape == want.shape == (n, 3, 8 * h, 8 * w) and torch.isfinite(got).all()
    rel, mx = _err(got, want)
    print(f"vae highres decode {name} {h}x{w}: rel-RMS {rel:.3e} max {mx:.3e}")
    assert rel <= 4e-3 and mx <= 4.2e-3, (rel, mx)           # measured 1.8e-3 / 1.9e-3 (SD-1.5 shape), 1.8e-3 / 2.1e-3 (tiny)
    got2 = m.decode(z.cuda()).sample.float().cpu()          # cached program, deterministic
    assert torch.equal(got, got2)


@pytest.mark.gpu
def test_hip_vae_encode_highres_vs_oracle(hiplib):
    """One 512 x 768 image at the SD-1.5 shape: 6144 tokens in the encoder's mid block."""
    cfg = V.SD15_VAE
    m = vae.AutoencoderKL(**_cfg(cfg)).eval()
    shapes = dict(V.decoder_shapes(cfg))
    shapes.update(V.encoder_shapes(cfg))
    sd = synth.procedural_state_dict(shapes, 37)
    m.load_state_dict(sd)
    m = m.to("cuda")
    x = synth.normal_tensor("vae.sd15.px_hi", (1, 3, 512, 768), 38).clamp(-1, 1)
    dist = m.encode(x.cuda()).latent_dist
    with torch.no_grad():
        mean, logvar = V.vae_encode_moments(sd, cfg, x)
    for nm, got, want in (("mean", dist.mean, mean), ("logvar", dist.logvar, logvar)):
        got = got.float().cpu()
        assert got.shape == want.shape == (1, 4, 64, 96) and torch.isfinite(got).all()
        rel, _ = _err(got, want)
        print(f"vae highres encode sd15 {nm}: rel-RMS {rel:.3e}")
        assert rel <= 3.5e-3, (nm, rel)                      # measured 1.7e-3 (mean), 1.5e-3 (logvar)
    again = m.encode(x.cuda()).latent_dist                   # cached program, deterministic
    assert torch.equal(again.mean, dist.mean) and torch.equal(again.logvar, dist.logvar)


_CHILD = """
import sys, torch
from oracle import vae_oracle as V
from rcdms_amd import switches, synth, vae
assert switches.VAE_FLASH == "1"
cfg = dict(V.SD15_VAE); cfg["norm_num_groups"] = cfg.pop("groups")
m = vae.AutoencoderKLDecoder(**cfg).eval()
m.load_state_dict(synth.procedural_state_dict(V.decoder_shapes(V.SD15_VAE), 31))
m = m.to("cuda")
z = synth.normal_tensor("vae.sd15.z", (1, 4, 32, 32), 32)
got = m.decode(z.cuda()).sample.float().cpu()
tags = m._programs[(1, 32, 32)][1].plan.tags
assert any(t.startswith("flash_attn ") for t in tags) and not any(t.startswith("softmax_rows") for t in tags), tags
assert torch.equal(got, m.decode(z.cuda()).sample.float().cpu())
torch.save(got, sys.argv[1])
"""


@pytest.mark.gpu
def test_the_two_forms_agree_at_32x32(hiplib, tmp_path):
    """SD-1.5 decode of 32 x 32 latents (1024 tokens, where both forms run): the flash form, forced with RCDM_VAE_FLASH=1
    in a child process (switches are read at import), meets the decode bounds against the oracle, and is within the
    rel-RMS bound of the default form's output."""
    m, sd = _decoder(V.SD15_VAE)
    z = synth.normal_tensor("vae.sd15.z", (1, 4, 32, 32), 32)
    default = m.decode(z.cuda()).sample.float().cpu()
    assert any(t.startswith("softmax_rows") for t in m._programs[(1, 32, 32)][1].plan.tags)
    path = str(tmp_path / "flash.pt")
    env = dict(os.environ)
    env["RCDM_VAE_FLASH"] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _CHILD, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    flash = torch.load(path)
    with torch.no_grad():
        want = V.vae_decode(sd, V.SD15_VAE, z)
    rel, mx = _err(flash, want)
    rel_forms, _ = _err(flash, default)
    print(f"vae sd15 32x32 flash form: rel-RMS {rel:.3e} max {mx:.3e}; vs the default form rel-RMS {rel_forms:.3e}")
    assert rel <= 4e-3 and mx <= 4.2e-3, (rel, mx)           # measured 1.8e-3 / 1.9e-3
    assert rel_forms <= 4e-3, rel_forms                      # measured 1.8e-3


# ---------------------------------------------------------------------------------------------- GPU: the pipeline
def _pipeline():
    from oracle import unet_oracle as O  # noqa: F401
    from rcdms_amd import context
    from rcdms_amd.scheduler import DDIMScheduler
    from rcdms_amd.vae import AutoencoderKL
    from src.pipelines.RCDMs_pipeline import RCDMsPipeline
    from tests.test_hip_unet import build
    from tests.test_pipeline_e2e import D, _Text, _Tok
    unet = build("unet_tiny")
    local = context.fine_stack(text_dim=D, vis_dim=32, hidden_dim=D, num_heads=8)
    glob = context.semantic_stack(text_dim=D, vis_dim=24, hidden_dim=D, num_heads=8)
    local.load_state_dict(synth.procedural_state_dict({k: v.shape for k, v in local.state_dict().items()}, 11))
    glob.load_state_dict(synth.procedural_state_dict({k: v.shape for k, v in glob.state_dict().items()}, 12))
    vcfg = V.tiny_vae_config()
    shapes = dict(V.decoder_shapes(vcfg))
    shapes.update(V.encoder_shapes(vcfg))
    sd_vae = synth.procedural_state_dict(shapes, 13)
    m = AutoencoderKL(**_cfg(vcfg)).eval()
    m.load_state_dict(sd_vae)
    pipe = RCDMsPipeline(vae=m, text_encoder=_Text(), tokenizer=_Tok(), unet=unet, local_module=local, global_module=glob,
                         scheduler=DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear")).to("cuda")
    return pipe, sd_vae, vcfg


@pytest.mark.gpu
def test_pipeline_512x576_runs_and_repeats(hiplib):
    """height = 512, width = 576: latents of 64 x 72 = 4608 tokens, set up as
    test_pipeline_five_captions_matches_oracle_flow[hip_vae]; the encode of the source frames raised NotImplementedError
    before the flash form."""
    pipe, _, _ = _pipeline()
    dev, H, W = "cuda", 512, 576
    caps = ["pororo waves", "loopy sings", "eddy builds", "crong jumps", "poby fishes"]
    src = synth.normal_tensor("e2e.src_hi", (5, 3, H, W), 2) * 0.5
    mask_label = torch.zeros(1, 5, H // 8, W // 8)
    mask_label[:, 0] = 1.0
    img1 = synth.normal_tensor("e2e.img1", (1, 9, 32), 3)
    proj0 = synth.normal_tensor("e2e.proj0", (4, 1, 24), 4)
    lat0 = synth.normal_tensor("e2e.lat_hi", (1, 4, 5, H // 8, W // 8), 5)

    def run():
        gen = torch.Generator(device=dev).manual_seed(9)
        return pipe(caps, src.to(dev), image_embeds_1=img1.to(dev), proj_embeds_0=proj0.to(dev),
                    mask_label=mask_label.to(dev), video_length=5, height=H, width=W, num_inference_steps=2,
                    guidance_scale=2.0, latents=lat0.to(dev), generator=gen).videos

    out = run()
    assert tuple(out.shape) == (1, 3, 5, H, W) and torch.isfinite(torch.as_tensor(out)).all()
    assert torch.equal(torch.as_tensor(out), torch.as_tensor(run()))


@pytest.mark.gpu
def test_pipeline_decode_latents_512x576_vs_oracle(hiplib):
    pipe, sd_vae, vcfg = _pipeline()
    lat = synth.normal_tensor("e2e.dec_hi", (1, 4, 5, 64, 72), 6)
    got = torch.as_tensor(pipe.decode_latents(lat.cuda())).float()
    zf = (lat / 0.18215).permute(0, 2, 1, 3, 4).reshape(5, 4, 64, 72)
    with torch.no_grad():
        want = V.vae_decode(sd_vae, vcfg, zf)
    want = (want.reshape(1, 5, 3, 512, 576).permute(0, 2, 1, 3, 4) / 2 + 0.5).clamp(0, 1)
    assert got.shape == want.shape
    rel, mx = _err(got, want)
    print(f"pipeline decode_latents 512x576: rel-RMS {rel:.3e} max {mx:.3e}")
    assert rel <= 4e-3 and mx <= 4.2e-3, (rel, mx)           # measured 5.8e-4 / 3.1e-3
