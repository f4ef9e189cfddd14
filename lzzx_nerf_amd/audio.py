"""Audio conditioning front-end on device: `NeRFNetwork.encode_audio` (/root/reference/nerf_triplane/network.py:226-240), i.e.
`AudioNet` (network.py:40-70) + `AudioAttNet` (network.py:9-37), as ONE kernel launch (csrc/lz_audio.hip).

Consumes the reference's state_dict keys unchanged: `audio_net.encoder_conv.{0,2,4,6}.{weight,bias}`,
`audio_net.encoder_fc1.{0,2}.{weight,bias}`, `audio_att_net.attentionConvNet.{0,2,4,6,8}.{weight,bias}`,
`audio_att_net.attentionNet.0.{weight,bias}`.
"""
import ctypes as C

import torch

from . import _lib
from ._util import call, ptr, stream


class FusedAudioEncoder:
    def __init__(self, state_dict, device="cuda"):
        self.device = torch.device(device)
        g = lambda k: state_dict[k].detach().to(self.device, torch.float32).contiguous()
        self.cw = [g("audio_net.encoder_conv.%d.weight" % i) for i in (0, 2, 4, 6)]
        self.cb = [g("audio_net.encoder_conv.%d.bias" % i) for i in (0, 2, 4, 6)]
        self.fw = [g("audio_net.encoder_fc1.%d.weight" % i) for i in (0, 2)]
        self.fb = [g("audio_net.encoder_fc1.%d.bias" % i) for i in (0, 2)]
        self.use_att = "audio_att_net.attentionNet.0.weight" in state_dict      # opt.att > 0 (network.py:124-126)
        if self.use_att:
            self.aw = [g("audio_att_net.attentionConvNet.%d.weight" % i) for i in (0, 2, 4, 6, 8)]
            self.ab = [g("audio_att_net.attentionConvNet.%d.bias" % i) for i in (0, 2, 4, 6, 8)]
            self.lw, self.lb = g("audio_att_net.attentionNet.0.weight"), g("audio_att_net.attentionNet.0.bias")
        self.dim_in, self.dim_aud = self.cw[0].shape[1], self.fw[1].shape[0]
        if tuple(self.cw[0].shape) != (32, self.dim_in, 3) or tuple(self.cw[3].shape) != (64, 64, 3) or self.dim_aud > 64:
            raise RuntimeError("FusedAudioEncoder expects the reference's AudioNet layout (network.py:45-60)")

    def _params(self, n_win):
        """lz_audio_params over this object's weights"""
        p = _lib.AudioParams()
        for i in range(4):
            p.c_w[i], p.c_b[i] = self.cw[i].data_ptr(), self.cb[i].data_ptr()
        for i in range(2):
            p.fc_w[i], p.fc_b[i] = self.fw[i].data_ptr(), self.fb[i].data_ptr()
        if self.use_att:
            for i in range(5):
                p.ac_w[i], p.ac_b[i] = self.aw[i].data_ptr(), self.ab[i].data_ptr()
            p.al_w, p.al_b = self.lw.data_ptr(), self.lb.data_ptr()
        p.dim_in, p.dim_aud, p.n_win, p.use_att = self.dim_in, self.dim_aud, n_win, int(self.use_att)
        return p

    SMOOTH_LIPS_LAMBDA = 0.35   # renderer.py:254-258, 456-460

    @torch.no_grad()
    def encode_track(self, features, att_mode, start=0, count=None, smooth_lips=False, enc_a_prev=None):
        """The codes of frames [start, start + count) of a clip from its whole feature track [T, dim_in, 16] (count None: to the end of the
        track) -> [count, dim_aud].  Row k has the bits of `self(pipeline.audio_window(features, att_mode, start + k))`, but AudioNet runs
        once per row of the track instead of once per frame and window (csrc/lz_audio.hip).  smooth_lips: the rows are
        blended along the clip as TalkingHeadFrame.render blends them frame by frame, 0.35 * previous + 0.65 * own, starting from
        enc_a_prev [1, dim_aud] (None: frame `start` keeps its own code)."""
        from .pipeline import audio_track_windows
        features = features.to(self.device, torch.float32).contiguous()
        if features.dim() != 3 or features.shape[1] != self.dim_in or features.shape[2] != 16:
            raise RuntimeError("audio features must be [T, %d, 16]" % self.dim_in)
        T, att_mode, start = features.shape[0], int(att_mode), int(start)
        n_win = audio_track_windows(T, att_mode).shape[1]                 # NotImplementedError for an att_mode outside 0, 1, 2
        if self.use_att and self.lw.shape[0] != n_win:                   # att_mode 0 hands an attention net one window
            raise RuntimeError("AudioAttNet was built for %d windows, got %d" % (self.lw.shape[0], n_win))
        if not self.use_att and att_mode != 0:
            raise RuntimeError("att_mode %d needs an attention net (audio_att_net.* is not in the state dict)" % att_mode)
        count = T - start if count is None else int(count)
        if start < 0 or count < 0 or start + count > T:
            raise RuntimeError("frames [%d, %d) are not inside the track of %d" % (start, start + count, T))
        out = torch.empty(count, self.dim_aud, dtype=torch.float32, device=self.device)
        if count == 0:
            return out
        w_prev = w_cur = 0.0
        if smooth_lips:
            w_prev, w_cur = self.SMOOTH_LIPS_LAMBDA, 1 - self.SMOOTH_LIPS_LAMBDA      # rounded to f32 on the way into the call
            if enc_a_prev is not None:
                enc_a_prev = enc_a_prev.to(self.device, torch.float32).reshape(-1).contiguous()
                if enc_a_prev.numel() != self.dim_aud:
                    raise RuntimeError("enc_a_prev must have %d elements" % self.dim_aud)
        else:
            enc_a_prev = None
        p = self._params(n_win)
        nbytes = _lib.load().lz_audio_track_workspace(count, self.dim_in, self.dim_aud)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        call("lz_audio_encode_track", C.byref(p), ptr(features), T, att_mode, start, count, w_prev, w_cur, ptr(enc_a_prev), ptr(out), ptr(ws),
             stream())
        return out

    @torch.no_grad()
    def forward(self, a):
        """a: [n_win, dim_in, 16] audio feature windows (n_win = 8 with attention, 1 without).  Returns enc_a [1, dim_aud]
        (attention) or [n_win, dim_aud]."""
        a = a.to(self.device, torch.float32).contiguous()
        n = a.shape[0]
        if a.dim() != 3 or a.shape[1] != self.dim_in or a.shape[2] != 16:
            raise RuntimeError("audio features must be [n_win, %d, 16]" % self.dim_in)
        if self.use_att and self.lw.shape[0] != n:
            raise RuntimeError("AudioAttNet was built for %d windows, got %d" % (self.lw.shape[0], n))
        p = self._params(n)
        out = torch.empty((1 if self.use_att else n), self.dim_aud, dtype=torch.float32, device=self.device)
        ws = torch.empty(n * 256, dtype=torch.float32, device=self.device) if self.dim_in >= 128 else None
        call("lz_audio_encode", C.byref(p), ptr(a), ptr(out), ptr(ws), stream())
        return out

    __call__ = forward
