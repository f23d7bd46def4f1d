"""Host restatements of the split-row formats and of the x8 GEMM's arithmetic, shared by the kernel tests (a plain
helper module)."""
import torch

from text2human_amd import ops


def e4m3(x):
    return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def x8_planes_host(x, s):
    """(hi, h8, l8) as the numbers they stand for: hi = fp16(x), h8 = e4m3(hi s) / s, l8 = e4m3((x - hi) 2048 s) / s"""
    hi = x.half().float()
    return hi, e4m3(hi * s) / s, e4m3((x - hi) * 2048.0 * s) / s


def emulate_x8(a, w, sa, sw):
    """the kernel's arithmetic in fp64: ah.bh + (ah8.bl8 + al8.bh8) / 2048"""
    ah, ah8, al8 = [t.double() for t in x8_planes_host(a, sa)]
    bh, bh8, bl8 = [t.double() for t in x8_planes_host(w, sw)]
    return ah @ bh.t() + (ah8 @ bl8.t() + al8 @ bh8.t()) / 2048.0


def pack_vt_host(v, B, T, H):
    """fp32 v [B*T, H*64] -> Vt [B][H][2][64][T] (int16 view) in the kernel's key order"""
    vt = v.view(B, T, H, 64).permute(0, 2, 3, 1).contiguous()          # [B, H, 64, T]
    pl = torch.stack(ops.split_planes_host(vt)).permute(1, 2, 0, 3, 4).contiguous()  # [B, H, 2, 64, T]
    out = torch.empty_like(pl)
    out[..., ops.vt_key_positions(T)] = pl
    return out.view(torch.int16)


def x8_rows_host(w, scale):
    """[rows, C] fp32 -> x8 rows [rows][C/32][hi16 (64 B) | hi8 (32 B) | lo8 (32 B)] as int16 [rows, C/32, 2, 32]"""
    r, C = w.shape
    hi = w.half()
    lo = (w - hi.float()) * ops.SPLIT_LO_SCALE
    out = torch.empty((r, C // 32, 128), dtype=torch.uint8)
    out[:, :, :64] = hi.view(r, C // 32, 32).view(torch.uint8).view(r, C // 32, 64)
    out[:, :, 64:96] = (hi.float() * scale).to(torch.float8_e4m3fn).view(torch.uint8).view(r, C // 32, 32)
    out[:, :, 96:] = (lo * scale).to(torch.float8_e4m3fn).view(torch.uint8).view(r, C // 32, 32)
    return out.view(torch.int16).view(r, C // 32, 2, 32)
