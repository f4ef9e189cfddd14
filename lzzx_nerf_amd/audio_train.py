"""Audio encoder for TRAINING: `NeRFNetwork.encode_audio` (nerf_triplane/network.py:226-240), i.e. `AudioNet`
(network.py:40-70) and, with attention, `AudioAttNet` (network.py:9-37), with the gradients the reference's head-stage step gives their
parameters (`run_cuda` encodes the audio with gradients on, renderer.py:252; `get_params` hands both nets to the optimizer, network.py:333,
344).

`FusedAudioTrainNet` keeps the reference's parameters, state-dict keys and default initialisation, so a checkpoint moves between it, the
reference, `audio.FusedAudioEncoder` and `pipeline.TalkingHeadFrame` unchanged.  Its forward is `lz_audio_encode` (csrc/lz_audio.hip): the
inference kernel's bits.  Its backward is two launches (csrc/lz_audio_train.hip) that recompute the forward and write every weight and bias
gradient with fixed-order sums (the same bits on every call, no host synchronisation)."""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from ._util import call, ptr, stream

SEQ_LEN = 8   # AudioAttNet's seq_len (network.py:10): the number of windows with attention


def _conv_stack(chans, stride):
    """Conv1d(k 3, padding 1) + LeakyReLU(0.02) pairs: parameters at Sequential indices 0, 2, 4, ... as in the reference"""
    layers = []
    for ci, co in zip(chans[:-1], chans[1:]):
        layers += [nn.Conv1d(ci, co, kernel_size=3, stride=stride, padding=1, bias=True), nn.LeakyReLU(0.02, True)]
    return nn.Sequential(*layers)


class AudioNet(nn.Module):
    """parameter container of network.py:40-70: encoder_conv.{0,2,4,6} (dim_in -> 32 -> 32 -> 64 -> 64, stride 2), encoder_fc1.{0,2}"""

    def __init__(self, dim_in, dim_aud):
        super().__init__()
        self.encoder_conv = _conv_stack((dim_in, 32, 32, 64, 64), 2)
        self.encoder_fc1 = nn.Sequential(nn.Linear(64, 64), nn.LeakyReLU(0.02, True), nn.Linear(64, dim_aud))


class AudioAttNet(nn.Module):
    """parameter container of network.py:9-37: attentionConvNet.{0,2,4,6,8} (dim_aud -> 16 -> 8 -> 4 -> 2 -> 1), attentionNet.0"""

    def __init__(self, dim_aud, seq_len=SEQ_LEN):
        super().__init__()
        self.attentionConvNet = _conv_stack((dim_aud, 16, 8, 4, 2, 1), 1)
        self.attentionNet = nn.Sequential(nn.Linear(seq_len, seq_len), nn.Softmax(dim=1))


def _params(mod, att, n, dim_in, dim_aud):
    p = _lib.AudioParams()
    cv, fc = mod.audio_net.encoder_conv, mod.audio_net.encoder_fc1
    for i in range(4):
        p.c_w[i], p.c_b[i] = cv[2 * i].weight.data_ptr(), cv[2 * i].bias.data_ptr()
    for i in range(2):
        p.fc_w[i], p.fc_b[i] = fc[2 * i].weight.data_ptr(), fc[2 * i].bias.data_ptr()
    if att:
        ac, al = mod.audio_att_net.attentionConvNet, mod.audio_att_net.attentionNet[0]
        for i in range(5):
            p.ac_w[i], p.ac_b[i] = ac[2 * i].weight.data_ptr(), ac[2 * i].bias.data_ptr()
        p.al_w, p.al_b = al.weight.data_ptr(), al.bias.data_ptr()
    p.dim_in, p.dim_aud, p.n_win, p.use_att = dim_in, dim_aud, n, int(att)
    return p


class _AudioEncode(Function):
    """a [n_win, dim_in, 16] (data: no gradient) -> enc_a; the parameters come after it in FusedAudioTrainNet._tensors() order"""

    @staticmethod
    def forward(ctx, mod, a, *weights):
        n = a.shape[0]
        out = torch.empty((1 if mod.att else n), mod.dim_aud, dtype=torch.float32, device=a.device)
        # the wide first layer's output (dim_in >= 128) stays in the workspace for the backward
        ws = torch.empty(n * 256, dtype=torch.float32, device=a.device) if mod.dim_in >= 128 else None
        p = _params(mod, mod.att, n, mod.dim_in, mod.dim_aud)
        call("lz_audio_encode", C.byref(p), ptr(a), ptr(out), ptr(ws), stream())
        ctx.mod, ctx.ws = mod, ws
        ctx.save_for_backward(a, *weights)
        return out

    @staticmethod
    def backward(ctx, g_out):
        a, *weights = ctx.saved_tensors
        mod, n = ctx.mod, a.shape[0]
        grads = [torch.empty_like(w) for w in weights]   # every element is written by the kernels
        g = _lib.AudioGrads()
        for i in range(4):
            g.g_c_w[i], g.g_c_b[i] = grads[2 * i].data_ptr(), grads[2 * i + 1].data_ptr()
        for i in range(2):
            g.g_fc_w[i], g.g_fc_b[i] = grads[8 + 2 * i].data_ptr(), grads[9 + 2 * i].data_ptr()
        if mod.att:
            for i in range(5):
                g.g_ac_w[i], g.g_ac_b[i] = grads[12 + 2 * i].data_ptr(), grads[13 + 2 * i].data_ptr()
            g.g_al_w, g.g_al_b = grads[22].data_ptr(), grads[23].data_ptr()
        p = _params(mod, mod.att, n, mod.dim_in, mod.dim_aud)
        go = g_out.float().contiguous()
        ws = torch.empty(_lib.load().lz_audio_train_workspace() // 4, dtype=torch.float32, device=a.device)
        call("lz_audio_train_backward", C.byref(p), ptr(a), ptr(ctx.ws), ptr(go), C.byref(g), ptr(ws), stream())
        return (None, None) + tuple(grads)


class FusedAudioTrainNet(nn.Module):
    """`NeRFNetwork.encode_audio` with its backward, as one forward launch (two for dim_in >= 128) and two backward launches.

    dim_in: 29 (deepspeech), 44 (esperanto), 1024 (hubert) or any other width; dim_aud <= 64 (the reference uses 32); att: the reference's
    opt.att > 0 (AudioAttNet over 8 windows).  Parameters `audio_net.*` and `audio_att_net.*` carry the reference's names, shapes and
    default (torch) initialisation.  Every call reads the live parameters (no packed copies: writes through `.data`, as the reference's EMA
    does, are seen by the next call).

    Precision: f32 always.  Under `autocast` the kernels still compute in f32 -- wider than the reference's `-O` mode, whose Conv1d / Linear
    run in half precision.  Every gradient is linear in the upstream one, so a GradScaler's power-of-two scale passes through exactly.
    No gradient flows to the audio features (data in train_step).  The `emb` path (nn.Embedding over class ids) is not supported."""

    def __init__(self, dim_in=29, dim_aud=32, att=True, emb=False):
        super().__init__()
        if emb:
            raise NotImplementedError("FusedAudioTrainNet: the emb path (nn.Embedding on audio class ids, network.py:119-120) is not supported")
        if not 1 <= dim_aud <= 64 or dim_in < 1:
            raise ValueError("FusedAudioTrainNet: dim_in >= 1 and 1 <= dim_aud <= 64")
        self.dim_in, self.dim_aud, self.att = int(dim_in), int(dim_aud), bool(att)
        self.audio_net = AudioNet(self.dim_in, self.dim_aud)
        if self.att:
            self.audio_att_net = AudioAttNet(self.dim_aud)

    def _tensors(self):
        cv, fc = self.audio_net.encoder_conv, self.audio_net.encoder_fc1
        t = [x for i in range(4) for x in (cv[2 * i].weight, cv[2 * i].bias)] + [x for i in range(2) for x in (fc[2 * i].weight, fc[2 * i].bias)]
        if self.att:
            ac, al = self.audio_att_net.attentionConvNet, self.audio_att_net.attentionNet[0]
            t += [x for i in range(5) for x in (ac[2 * i].weight, ac[2 * i].bias)] + [al.weight, al.bias]
        return t

    def forward(self, a):
        """a: [n_win, dim_in, 16] audio feature windows (8 with attention).  Returns enc_a [1, dim_aud] (attention) or [n_win, dim_aud]."""
        ts = self._tensors()
        dev = ts[0].device
        if dev.type != "cuda":
            raise RuntimeError("FusedAudioTrainNet runs on the GPU: move the module to a cuda device")
        if a.dim() != 3 or a.shape[1] != self.dim_in or a.shape[2] != 16:
            raise RuntimeError("audio features must be [n_win, %d, 16]" % self.dim_in)
        n = a.shape[0]
        if self.att and n != SEQ_LEN:
            raise RuntimeError("AudioAttNet was built for %d windows, got %d" % (SEQ_LEN, n))
        if not 1 <= n <= 8:
            raise RuntimeError("1..8 audio windows, got %d" % n)
        if any(t.dtype != torch.float32 or not t.is_contiguous() for t in ts):
            raise RuntimeError("FusedAudioTrainNet keeps f32 contiguous parameters")
        with torch.autocast(device_type="cuda", enabled=False):
            a = a.detach().to(dev, torch.float32).contiguous()
            return _AudioEncode.apply(self, a, *ts)

    def param_groups(self, lr_net, wd=0):
        """the optimizer groups NeRFNetwork.get_params gives these nets (network.py:333, 344): audio_net at lr_net / wd, audio_att_net at
        5 lr_net with weight decay 1e-4"""
        groups = [{"params": list(self.audio_net.parameters()), "lr": lr_net, "weight_decay": wd}]
        if self.att:
            groups.append({"params": list(self.audio_att_net.parameters()), "lr": lr_net * 5, "weight_decay": 0.0001})
        return groups
