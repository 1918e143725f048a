"""FusedSeparableBlock hands tensors to and from its convolutions through arguments and return values: a block forward leaves
no new attribute on a module.  CPU only: the ops entry points are stubs."""
import torch

from epn_pointcloud_amd import ops, schedule as S


def test_block_forward_leaves_no_attribute_on_its_convolutions(monkeypatch):
    b, c, p, a = 2, 32, 8, 60
    seen = {}

    def inter(feats, W, geo, out_dtype=None, share_input=False):
        seen["share_input"] = share_input
        out = torch.zeros(b, c, p, a)
        return (out, feats, torch.ones(3)) if share_input else out

    def intra(feats, W, idx, pre_norm=None, pre_part=None, out_stats=False, pre_eval=False):
        seen["intra"] = (pre_norm, pre_part, out_stats)
        out = torch.zeros(b, c, p, a)
        return (out, torch.ones(5)) if out_stats else out

    def pair(xa, norm_a, xb, norm_b, conv_bias_b=None, slope=0.01, part_b=None, part_a=None):
        seen["pair"] = (part_b, part_a)
        return xa + xb

    monkeypatch.setattr(ops, "inter_so3conv", inter)
    monkeypatch.setattr(ops, "intra_so3conv", intra)
    monkeypatch.setattr(ops, "norm_act_pair", pair)
    monkeypatch.setattr(ops, "conv1x1", lambda x, w, bias=None, col_stats=False, x_amax=None:
                        (torch.zeros(b, c, p, a), torch.ones(7)) if col_stats else torch.zeros(b, c, p, a))
    blk = S.FusedSeparableBlock(S.Layer(c, c, 1, 0.4, 0.08, 4, True)).train()
    monkeypatch.setattr(blk.intra_conv.conv, "takes_spectral_form", lambda is_cuda=True: True)   # the norm-on-load route
    conv, iconv = blk.inter_conv.conv, blk.intra_conv.conv
    iconv._idx32()                                     # the module's own cache of its index table
    before = set(conv.__dict__), set(iconv.__dict__)
    x = S.zptk.SphericalPointCloud(torch.zeros(b, 3, p), torch.zeros(b, c, p, a), None)
    out = blk(x, torch.zeros(b, p, 4, dtype=torch.int32), torch.zeros(b, p, a, conv.kernel_size, 4))
    assert len(out) == 4 and out[3].feats.shape == (b, c, p, a)
    assert seen["share_input"] is True
    assert seen["intra"][0] is blk.inter_conv.norm and seen["intra"][1].numel() == 3 and seen["intra"][2] is True
    assert seen["pair"][0].numel() == 7 and seen["pair"][1].numel() == 5
    assert (set(conv.__dict__), set(iconv.__dict__)) == before
    # without the flags: the reference's return values
    assert len(conv(x, torch.zeros(b, p, 4, dtype=torch.int32), torch.zeros(b, p, a, conv.kernel_size, 4))) == 4
    assert isinstance(iconv(x), S.zptk.SphericalPointCloud)
