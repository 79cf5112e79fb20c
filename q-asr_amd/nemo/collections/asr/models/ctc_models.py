"""EncDecCTCModel: preprocessor -> ConvASREncoder -> ConvASRDecoder -> greedy argmax
(nemo/collections/asr/models/ctc_models.py:43-147, 383-406), without the NeMo-core / Lightning layers.

Two execution paths share this one object:
  * host PyTorch (calibration with running ranges, dynamic mode, `--no_quant`): the modules' own forward;
  * the HIP engine: once every QuantAct is frozen (`qm.evaluate`), non-dynamic, symmetric and the BNs are
    folded, forward() packs the model once (qasr.pack) and runs mel front-end + encoder + decoder in the
    gfx950 kernels of libqasr_hip.so.  There is no CPU fallback for that configuration: a missing
    library or GPU raises.
"""
import dataclasses
import io
import os
import tarfile

import numpy as np
import torch
import torch.nn as nn
import yaml

from nemo.collections.asr.modules.audio_preprocessing import AudioToMelSpectrogramPreprocessor
from nemo.collections.asr.modules.conv_asr import ConvASRDecoder, ConvASREncoder
from nemo.collections.asr.parts.jasper import MaskedConv1d
from nemo.quantization.utils.quant_modules import QuantAct
from qasr import configs as qconfigs
from qasr import synth, topology

_MODEL_CONFIG, _MODEL_WEIGHTS = "model_config.yaml", "model_weights.ckpt"


def _strip_target(d):
    return {k: v for k, v in d.items() if k not in ('_target_', 'cls', 'params')}


class EncDecCTCModel(nn.Module):
    def __init__(self, cfg, trainer=None):
        super().__init__()
        cfg = dict(cfg.get('model', cfg))
        enc, dec = dict(cfg['encoder']), dict(cfg['decoder'])
        # the fork hard-wires symmetric quantisation into both halves (ctc_models.py:103-107)
        enc['quant_mode'] = dec['quant_mode'] = 'symmetric'
        self.cfg = cfg
        self._cfg = cfg
        self.preprocessor = AudioToMelSpectrogramPreprocessor(**_strip_target(cfg['preprocessor']))
        self.encoder = ConvASREncoder(**_strip_target(enc))
        if dec.get('vocabulary') is None:
            dec['vocabulary'] = cfg.get('labels')
        self.decoder = ConvASRDecoder(**_strip_target(dec))
        self.spec_augmentation = None
        self._test_dl = None
        self._engine = None
        self._engine_key = None
        self._reserve = None                 # (max_batch, max_seconds) after reserve()
        self._ragged_engine = None           # the reserved engine of the current quantiser state / device
        self._ragged_key = None
        self._ragged_warned = False
        self._reserve_logp = True            # decode_long's own greedy reservation keeps no log-probabilities
        self._quant_version = 0
        self.resample_quality = 'best'       # filter preset of forward(..., sample_rate=): 'best' or 'fast' (qasr.resample)

    # ------------------------------------------------------------------ construction / checkpoints
    @classmethod
    def list_available_models(cls):
        return ['QuartzNet15x5Base-En', 'QuartzNet15x5Base-Zh', 'Jasper10x5Dr-En']

    @classmethod
    def restore_from(cls, restore_path, map_location='cpu', strict=False):
        """.nemo = tar(.gz){model_config.yaml, model_weights.ckpt} (nemo/core/classes/modelPT.py:40-41,379-400)."""
        if not os.path.exists(restore_path):
            raise FileNotFoundError(f"Can't find {restore_path}")
        with tarfile.open(restore_path, 'r:*') as tar:
            names = {os.path.basename(m.name): m for m in tar.getmembers()}
            cfg = yaml.safe_load(tar.extractfile(names[_MODEL_CONFIG]).read())
            blob = tar.extractfile(names[_MODEL_WEIGHTS]).read()
        model = cls(cfg)
        sd = torch.load(io.BytesIO(blob), map_location=map_location, weights_only=True)
        model.load_state_dict(sd, strict=strict)
        return model

    def save_to(self, save_path):
        with tarfile.open(save_path, 'w:gz') as tar:
            def add(name, data):
                ti = tarfile.TarInfo(name)
                ti.size = len(data)
                tar.addfile(ti, io.BytesIO(data))
            add(_MODEL_CONFIG, yaml.safe_dump(self.cfg).encode())
            buf = io.BytesIO()
            torch.save(self.state_dict(), buf)
            add(_MODEL_WEIGHTS, buf.getvalue())

    @classmethod
    def from_pretrained(cls, model_name, refresh_cache=False):
        """The reference downloads `<name>.nemo` from NGC (ctc_models.py:55-88); there is no network here, so the
        file is looked up under $QASR_MODEL_DIR (or ~/.cache/torch/NeMo)."""
        if model_name not in cls.list_available_models():
            raise FileNotFoundError(f"Model {model_name} was not found. Available: {cls.list_available_models()}")
        for root in (os.environ.get('QASR_MODEL_DIR'), os.path.expanduser('~/.cache/torch/NeMo')):
            if root:
                for dirpath, _, files in os.walk(root):
                    if model_name + '.nemo' in files:
                        return cls.restore_from(os.path.join(dirpath, model_name + '.nemo'))
        raise FileNotFoundError(f"{model_name}.nemo not found locally and this environment has no network; put the "
                                f"checkpoint under $QASR_MODEL_DIR or pass a .nemo path")

    @classmethod
    def from_synthetic(cls, model_name='QuartzNet15x5Base-En', seed=0):
        """Random-init model of the named architecture with the deterministic weights of qasr.synth."""
        model = cls(qconfigs.model_config(model_name))
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
              synth.make_state_dict(topology.MODELS[model_name](), seed).items()}
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        return model

    def load_state_dict(self, state_dict, strict=False):
        """strict=False by default like ModelPT (modelPT.py:400): the fork's extra buffers are absent from
        upstream checkpoints.  `...conv.weight` (QuantConv1d) is mirrored into the inner `...conv.conv.weight`."""
        sd = dict(state_dict)
        for k in list(sd):
            if k.endswith('.conv.weight') and k[:-len('weight')] + 'conv.weight' not in sd:
                sd[k[:-len('weight')] + 'conv.weight'] = sd[k]
        if 'decoder.decoder_layers.0.weight' in sd:
            sd.setdefault('decoder.decoder_layers.0.conv.weight', sd['decoder.decoder_layers.0.weight'])
            if 'decoder.decoder_layers.0.bias' in sd:
                sd.setdefault('decoder.decoder_layers.0.conv.bias', sd['decoder.decoder_layers.0.bias'])
        res = super().load_state_dict(sd, strict=strict)
        self._quant_state_changed()
        return res

    # ------------------------------------------------------------------ quantisation switches
    def set_quant_bit(self, quant_bit, mode='all'):
        self.encoder.set_quant_bit(quant_bit, mode)
        self.decoder.set_quant_bit(quant_bit, mode)
        self._quant_state_changed()

    def set_quant_mode(self, quant_mode):
        self.encoder.set_quant_mode(quant_mode)
        self.decoder.set_quant_mode(quant_mode)
        self._quant_state_changed()

    def _quant_state_changed(self):
        self._quant_version += 1
        if self._engine is not None:
            self._engine.close()
        self._engine = None
        if getattr(self, '_ragged_engine', None) is not None:
            self._ragged_engine.close()
        self._ragged_engine = None

    # ------------------------------------------------------------------ data
    def setup_test_data(self, test_data_config):
        from nemo.collections.asr.data.audio_to_text import make_dataloader
        cfg = dict(test_data_config)
        cfg.setdefault('shuffle', False)
        self._test_dl = make_dataloader(cfg)

    def test_dataloader(self):
        return self._test_dl

    @torch.no_grad()
    def transcribe(self, paths2audio_files, batch_size=4, logprobs=False, return_hypotheses=False, window_s=None,
                   overlap_s=4.0):
        """Greedy transcripts (or per-file log-probabilities) of audio files, in input order - the reference's debugging /
        prototyping entry (ctc_models.py:148-212, 476-503): dither off and pad_to 0 for the duration of the call, evaluation
        mode, a temporary manifest with `duration` 100000 and text 'nothing', batch size min(batch_size, #files), silence
        trimmed (`trim_silence: True`), everything restored afterwards.  A calibrated model runs on the HIP engine.
        return_hypotheses=True (an extension): qasr.ctc.Hypothesis objects - text, label and word times, confidences - from
        decode() instead of strings.  window_s=SECONDS (an extension, for long files): every batch goes through decode_long
        with windows of window_s that overlap by overlap_s (guard: a quarter of the overlap, at most 1 s) instead."""
        if paths2audio_files is None or len(paths2audio_files) == 0:
            return {}
        if window_s is not None and logprobs:
            raise ValueError('transcribe: window_s returns transcripts or hypotheses, not log-probabilities')
        import json
        import tempfile
        from nemo.collections.asr.data.audio_to_text import make_dataloader
        from nemo.collections.asr.metrics.wer import WER
        hypotheses = []
        mode = self.training
        device = next(self.parameters()).device
        f = self.preprocessor.featurizer
        dither_value, pad_to_value = f.dither, f.pad_to
        try:
            f.dither, f.pad_to = 0.0, 0
            self.eval()
            with tempfile.TemporaryDirectory() as tmpdir:
                manifest = os.path.join(tmpdir, 'manifest.json')
                with open(manifest, 'w') as fp:
                    for audio_file in paths2audio_files:
                        fp.write(json.dumps({'audio_filepath': audio_file, 'duration': 100000, 'text': 'nothing'}) + '\n')
                loader = make_dataloader({'manifest_filepath': manifest, 'sample_rate': 16000, 'labels': self.decoder.vocabulary,
                                          'batch_size': min(batch_size, len(paths2audio_files)), 'trim_silence': True,
                                          'shuffle': False})
                wer = WER(vocabulary=self.decoder.vocabulary)
                for batch in loader:
                    if window_s is not None:
                        hyps = self.decode_long(batch[0].to(device).float(), batch[1].to(device), window_s=window_s,
                                                overlap_s=overlap_s, guard_s=min(1.0, float(overlap_s) / 4))
                        hypotheses += hyps if return_hypotheses else [h.text for h in hyps]
                        continue
                    if return_hypotheses and not logprobs:
                        hypotheses += self.decode(input_signal=batch[0].to(device).float(),
                                                  input_signal_length=batch[1].to(device))
                        continue
                    logits, logits_len, greedy = self.forward(input_signal=batch[0].to(device).float(),
                                                              input_signal_length=batch[1].to(device))
                    if logprobs:
                        for idx in range(logits.shape[0]):
                            hypotheses.append(logits[idx][: logits_len[idx]])
                    else:
                        hypotheses += wer.ctc_decoder_predictions_tensor(greedy)
        finally:
            self.train(mode=mode)
            f.dither, f.pad_to = dither_value, pad_to_value
        return hypotheses

    # ------------------------------------------------------------------ engine path
    def _masked_convs(self):
        for blk in self.encoder.encoder_layers:
            yield from blk._masked_convs()

    def engine_ready(self):
        """True when the model is in the calibrated, frozen, folded, symmetric configuration the engine runs."""
        acts = [m for m in self.modules() if isinstance(m, QuantAct)]
        if not acts or any(a.quant_mode != 'symmetric' or a.running_stat or a.dynamic for a in acts):
            return False
        for blk in self.encoder.encoder_layers:
            if any(isinstance(l, nn.BatchNorm1d) for l in blk.mconv):
                return False                                    # BN not folded
        return all(mc.conv.fix_bn and mc.conv.quant_mode == 'symmetric' for mc in self._masked_convs())

    def dynamic_ready(self):
        """True when every QuantAct is in dynamic mode (qm.set_dynamic, quant_modules.py:149-167) on min / max or - all of
        them alike - percentile ranges (qm.set_percentile, :158-167) and the convs are folded and fixed: the configuration
        qasr.dynamic.DynamicRunner executes on the HIP kernels.  (Per-channel activation ranges are not a configuration the
        reference's QuantConv1d can run: int_conv multiplies [Cout,1,1] weight scales with [1,Cin,1] activation scales.)"""
        acts = [m for m in self.modules() if isinstance(m, QuantAct)]
        if not acts or any(a.quant_mode != 'symmetric' or not a.dynamic or a.per_channel for a in acts):
            return False
        if len({a.percentile or None for a in acts}) != 1:
            return False
        for blk in self.encoder.encoder_layers:
            if any(isinstance(l, nn.BatchNorm1d) for l in blk.mconv):
                return False
        return all(mc.conv.fix_bn and mc.conv.quant_mode == 'symmetric' for mc in self._masked_convs())

    def _get_dynamic_runner(self, device):
        """DynamicRunner for the live weights (both model families), or None if it declines the topology: such a model
        keeps the host modules in dynamic mode."""
        percentile = next(m for m in self.modules() if isinstance(m, QuantAct)).percentile or None
        key = ('dyn', self._quant_version, device.index or 0, percentile)
        if self._engine_key != key:
            from qasr import dynamic, engine as qengine
            qengine.load_library()
            cfg, sd, _, _, wbit, abit = self.export_pack_inputs()
            try:
                self._engine = dynamic.DynamicRunner(cfg, sd, wbit, abit, device, percentile=percentile)
            except NotImplementedError:
                self._engine = None
            self._engine_key = key
        return self._engine

    def export_pack_inputs(self):
        """(ModelCfg, pre-fold NeMo-keyed float state dict, act_min, act_max, wbit, abit) of the live model."""
        cfg = qconfigs.topology_from_config(self.cfg)
        plan = topology.conv_plan(cfg)
        sd, amin, amax = {}, [], []
        wbits, abits = set(), set()
        for blk, sites in zip(self.encoder.encoder_layers, plan):
            mcs = list(blk._masked_convs())
            assert len(mcs) == len(sites)
            for mc, s in zip(mcs, sites):
                sd[f'{s.key}.conv.weight'] = mc.conv.weight.detach().cpu().float()
                if mc.conv.bias is not None:
                    sd[f'{s.key}.conv.bias'] = mc.conv.bias.detach().cpu().float()
                if s.bn_key is not None:
                    bn = mc.conv.bn
                    assert bn is not None, f'{s.key}: call encoder.bn_folding() first'
                    for n in ('weight', 'bias', 'running_mean', 'running_var'):
                        sd[f'{s.bn_key}.{n}'] = getattr(bn, n).detach().cpu().float()
                amin.append(float(mc.act.x_min))
                amax.append(float(mc.act.x_max))
                wbits.add(mc.conv.weight_bit)
                abits.add(mc.act.activation_bit - (1 if mc.asymmetric else 0))
            amin.append(float(blk.res_act.x_min))
            amax.append(float(blk.res_act.x_max))
        q = self.decoder.decoder_layers[0]
        sd['decoder.decoder_layers.0.weight'] = q.weight.detach().cpu().float()
        sd['decoder.decoder_layers.0.bias'] = q.bias.detach().cpu().float()
        amin.append(float(self.decoder.act.x_min))
        amax.append(float(self.decoder.act.x_max))
        wbits.add(q.weight_bit)
        abits.add(self.decoder.act.activation_bit)
        if len(wbits) != 1 or len(abits) != 1:
            raise NotImplementedError(f'mixed bit-widths are not packed yet: weights {wbits}, activations {abits}')
        return cfg, sd, np.array(amin, np.float32), np.array(amax, np.float32), wbits.pop(), abits.pop()

    def _get_engine(self, device):
        key = (self._quant_version, device.index or 0)
        if self._engine is None or self._engine_key != key:
            from qasr import engine as qengine, pack
            qengine.load_library()                               # raises when the HIP extension is missing
            blob, self._pack_meta = pack.pack_model(*self.export_pack_inputs())
            self._engine = qengine.Engine(blob, device.index or 0)
            self._engine_key = key
        return self._engine

    def reserve(self, max_batch, max_seconds):
        """Ragged batches without allocation (an extension; qasr_engine_reserve): afterwards forward(), decode() and
        transcribe() of the calibrated model run every batch of at most `max_batch` utterances of at most `max_seconds`
        seconds through one reserved engine - buffers allocated once, one captured graph per length bucket - and return
        what they return without it (the results are copies: they stay valid across batches).  A batch outside the
        envelope takes the ordinary path, with one warning.  The engine is built on the first batch; reserve(None, None)
        drops the reservation."""
        if self._ragged_engine is not None:
            self._ragged_engine.close()
        self._ragged_engine = None
        self._ragged_warned = False
        if not max_batch or not max_seconds:
            self._reserve = None
            return self
        if int(max_batch) < 1 or float(max_seconds) <= 0:
            raise ValueError('reserve: max_batch >= 1 and max_seconds > 0')
        self._reserve = (int(max_batch), float(max_seconds))
        return self

    def _get_ragged_engine(self, device):
        """the reserved engine for the live weights on `device` (None: the front-end is not the HIP kernels' configuration)"""
        if not self._frontend_hip_supported():
            return None
        f = self.preprocessor.featurizer
        pad_to = int(f.pad_to) if 0 < int(f.pad_to) and 128 % int(f.pad_to) == 0 else 16
        want_logp = bool(getattr(self, '_reserve_logp', True))
        key = (self._quant_version, device.index or 0, self._reserve, pad_to, want_logp)
        if self._ragged_engine is None or self._ragged_key != key:
            from qasr import engine as qengine, pack, ragged
            qengine.load_library()
            if self._ragged_engine is not None:
                self._ragged_engine.close()
            blob, self._pack_meta = pack.pack_model(*self.export_pack_inputs())
            max_batch, max_seconds = self._reserve
            max_samples = int(round(max_seconds * self.preprocessor._sample_rate))
            eng = qengine.Engine(blob, device.index or 0)
            # both entries share the envelope: audio (pad_to > 0) and features (transcribe() runs with pad_to 0)
            eng.reserve(max_batch, max_samples=max_samples, max_frames=ragged.frontend_frames(max_samples, pad_to),
                        want_logp=want_logp, decode=True, n_mels=int(f.fb.shape[1]), pad_to=pad_to)
            self._ragged_engine, self._ragged_key = eng, key
        return self._ragged_engine

    def _ragged_forward(self, has_in, input_signal, input_signal_length, processed_signal, processed_signal_length, decode):
        """forward / decode of one batch on the reserved engine; None when the batch lies outside the envelope"""
        import dataclasses
        from qasr import ragged
        ref = input_signal if has_in else processed_signal
        eng = self._get_ragged_engine(ref.device)
        if eng is None:
            return None
        f = self.preprocessor.featurizer
        r = eng.reserved
        M = ragged.envelope_frames(r.max_samples, r.max_frames, r.pad_to)
        stream = torch.cuda.current_stream(ref.device)
        if stream.cuda_stream == 0:                              # graphs cannot be captured on the legacy default stream
            side = getattr(self, '_ragged_stream', None)
            if side is None or side.device != ref.device:
                side = self._ragged_stream = torch.cuda.Stream(ref.device)
            side.wait_stream(stream)
        else:
            side = stream
        out = None
        with torch.cuda.stream(side):
            if has_in and int(f.pad_to) == r.pad_to:
                if input_signal.shape[0] <= r.max_batch and 256 < input_signal.shape[1] <= r.max_samples:
                    sig = input_signal.float().contiguous()
                    if f.dither > 0:
                        sig = sig + f.dither * torch.randn_like(sig)
                    fb, plan = self._frontend_plan_for(ref.device)
                    audio_lens = input_signal_length.to(device=ref.device, dtype=torch.int32).contiguous()
                    window = f.window.to(device=ref.device, dtype=torch.float32).contiguous()
                    out = eng.forward_ragged_audio(sig, audio_lens, fb, window, plan, float(f.preemph), r.pad_to, stream=side)
            else:
                if has_in:
                    processed_signal, processed_signal_length = self._frontend_hip(input_signal, input_signal_length)
                if processed_signal.shape[0] <= r.max_batch and processed_signal.shape[2] <= M:
                    out = eng.forward_ragged(processed_signal.float(), processed_signal_length, stream=side)
            if out is not None:                                  # views of the engine's buffers: callers keep results across batches
                if decode == 'frames':                           # decode_long: (tokens, frame scores, encoded lengths)
                    out = (out[1].clone(), out[3].frame_score.clone(), out[2].clone())
                elif decode:
                    res = out[3]
                    out = dataclasses.replace(res, **{k: getattr(res, k).clone() for k in
                                                      ('labels', 'n_labels', 'start', 'nframes', 'score', 'utt_score', 'frame_score')})
                else:
                    out = (out[0].clone(), out[2].long(), out[1].long())
        if side is not stream:
            stream.wait_stream(side)
            if out is not None:                                  # allocated on the side stream, used on the caller's
                for t in (out if isinstance(out, tuple) else [getattr(out, fl.name) for fl in dataclasses.fields(out)]):
                    if torch.is_tensor(t):
                        t.record_stream(stream)
        return out

    def _frontend_hip_supported(self):
        """The HIP front-end kernels are built for the QuartzNet / Jasper preprocessor (quartznet_15x5.yaml:30-41):
        n_fft 512, hop 160, a 320-tap window, per-feature normalisation, log(x + 2^-24), power spectrum.  Any other
        featurizer configuration runs the host module on the GPU tensors instead - the same module calibration used -
        rather than silently producing different features (a shorter window would even be read out of bounds)."""
        f = self.preprocessor.featurizer
        return (f.n_fft == 512 and f.hop_length == 160 and f.win_length == 320 and f.window.numel() == 320
                and f.fb.dim() == 3 and f.fb.shape[2] == 257 and f.normalize == 'per_feature' and bool(f.log)
                and f.log_zero_guard_type == 'add' and not isinstance(f.log_zero_guard_value, str)
                and float(f.log_zero_guard_value) == 2.0 ** -24 and float(f.mag_power) == 2.0 and f.preemph is not None
                and f.pad_value == 0 and isinstance(f.pad_to, int) and f.pad_to >= 0)

    def _frontend_plan_for(self, device):
        """(filterbank on `device`, qasr_frontend_plan workspace): the filterbank-only tables, built once per model / device."""
        from qasr import engine as qengine
        f = self.preprocessor.featurizer
        fb = f.fb[0].to(device=device, dtype=torch.float32).contiguous()
        key = (fb.data_ptr(), f.fb._version, str(device))
        if getattr(self, '_frontend_plan_key', None) != key:
            self._frontend_plan = qengine.frontend_plan(fb)
            self._frontend_plan_key = key
        return self._frontend_plan._qasr_fb, self._frontend_plan

    def _frontend_hip(self, signal, length):
        from qasr import engine as qengine
        f = self.preprocessor.featurizer
        if not self._frontend_hip_supported():
            return self.preprocessor(input_signal=signal, length=length)
        if f.dither > 0:
            signal = signal + f.dither * torch.randn_like(signal)
        fb, plan = self._frontend_plan_for(signal.device)
        return qengine.frontend_mel(signal.float().contiguous(), length, fb, f.window.contiguous(), float(f.preemph),
                                    int(f.pad_to), plan=plan)

    # ------------------------------------------------------------------ forward
    def forward(self, input_signal=None, input_signal_length=None, processed_signal=None,
                processed_signal_length=None, sample_rate=None, channels=1):
        """sample_rate=R / channels=C (an extension): input_signal is PCM at R Hz - int16, interleaved when C > 1, or float -
        and input_signal_length counts frames at R; see _resample_in.  The defaults leave the call as it was."""
        input_signal, input_signal_length = self._resample_in(input_signal, input_signal_length, sample_rate, channels)
        return self._forward(input_signal, input_signal_length, processed_signal, processed_signal_length)

    def _resample_in(self, signal, length, sample_rate, channels):
        """forward / decode / align with sample_rate=R: the batch is brought to the model's rate first - on the device
        (k_resample, one launch on the current stream, lengths converted there) for cuda tensors, by the NumPy twin
        (qasr.resample.resample_host) otherwise - and the existing path runs on the float32 result, reserved engine and
        dynamic path included; reserve() keeps meaning seconds.  With sample_rate=None, or the model's own rate with a mono
        float signal, nothing here runs."""
        if sample_rate is None:
            if int(channels) != 1:
                raise ValueError('channels needs sample_rate (the rate of the interleaved PCM)')
            return signal, length
        if signal is None or length is None:
            raise ValueError('sample_rate describes input_signal / input_signal_length: give both')
        target = int(self.preprocessor._sample_rate)
        if int(sample_rate) == target and int(channels) == 1 and signal.is_floating_point():
            return signal, length
        from qasr import engine as qengine, resample as qresample
        key = (int(sample_rate), target, self.resample_quality)
        plans = self.__dict__.setdefault('_resample_plans', {})
        if key not in plans:
            plans[key] = qresample.ResamplePlan(sample_rate, target, self.resample_quality)      # refuses a rate by name
        if signal.dtype != torch.int16:
            signal = signal.float()
        out, out_lens = qengine.resample(signal, length, plans[key], channels=int(channels))
        return out, out_lens.to(length.dtype)

    def seconds_per_frame(self):
        """Seconds per encoder output frame, from the model itself: featurizer hop x the encoder's strides (0.02 s for the
        registered models)."""
        from qasr import ctc as qctc
        f = self.preprocessor.featurizer
        return qctc.seconds_per_frame(qconfigs.topology_from_config(self.cfg), f.hop_length / float(self.preprocessor._sample_rate))

    @torch.no_grad()
    def decode(self, input_signal=None, input_signal_length=None, processed_signal=None, processed_signal_length=None,
               beam_width=None, n_best=1, cutoff_top_n=40, lm=None, alpha=0.0, beta=0.0, timestamps=False, boost=None,
               boost_weight=1.0, sample_rate=None, channels=1, posteriors=False, _rows=False, mbr=None, mbr_scale=1.0):
        """Greedy CTC hypotheses of one batch (an extension of the reference's API): List[qasr.ctc.Hypothesis] with the
        text, every label's start / end time and confidence (best frame log-probability of its run), word groups and the
        log-probability of the greedy path.  Decoding stops at each utterance's encoded length.  On the static engine the
        collapse (k_ctc) and the per-frame scores ride inside the engine's call on persistent buffers - no log-prob tensor
        is written; on the dynamic device path and the host modules the scores are log_probs gathered at the tokens,
        collapsed by qasr_ctc_collapse (cuda) or qasr.ctc.collapse_host (cpu).

        beam_width=W (1 .. 128) replaces the greedy collapse by a CTC prefix beam search without a language model
        (qasr.beam): the forward runs with log-probabilities, then k_topn (the cutoff_top_n <= 64 best classes per frame)
        and k_beam follow on the same stream - on the static engine, a reserved engine and the dynamic path alike; the host
        modules run the NumPy twin.  The hypotheses carry text, labels and utt_score (the beam score).  A prefix has no
        single alignment, so their time lists are empty unless timestamps=True: then the n_best label rows of the beam are
        aligned against the same log-probabilities (the Viterbi alignment of qasr.align; one more launch, k_align, over the
        beam's device buffers as they lie) and start_s / end_s / score / words are filled as for greedy hypotheses;
        utt_score stays the beam score.  n_best > 1 (<= W) returns, per utterance, the list of its best hypotheses, best
        first.  posteriors=True (needs beam_width and timestamps=True) runs k_post behind k_align over the same rows, n_best
        problems per utterance, and fills post / post_min / word_post / frame_post of every aligned hypothesis as
        align(posteriors=True) does.

        lm=<path of an ARPA file, or a qasr.ngram.NgramLM> (needs beam_width) adds the n-gram model with the weights alpha
        (0 .. 16) and beta (|beta| <= 16) as ctc_decoders' Scorer does (qasr.beam.LM_RULES; k_beam_lm on the device): word
        mode if the vocabulary has a space, else character mode.  utt_score then includes the model's share, which the
        hypotheses also carry as lm_score.  A model loaded from a path is kept on the module, so a sweep of alpha / beta
        loads and packs once.  Out of scope: KenLM binary files, cutoff_prob < 1, </s> scoring, orders above 6.

        boost=<a list of phrases (text, or (text, weight) pairs), or a qasr.boost.PhraseSet> (needs beam_width) biases the
        search towards those phrases ("hot words"), with or without lm: every label of a matched phrase earns its weight
        in nats (boost_weight where a phrase has none, 0 .. 16), an unfinished match earns nothing, and with a vocabulary
        that has a space phrases match whole words only (qasr.boost.BOOST_RULES; k_beam_boost on the device, the NumPy twin
        on the host modules).  utt_score then includes the boosting's share, which the hypotheses also carry as
        boost_score.  The list changes per call: it is compiled and packed here, per call.

        mbr='word' | 'char' (needs beam_width and n_best >= 2) re-ranks every utterance's n-best list by minimum Bayes risk
        (qasr.mbr.MBR_RULES): the row with the fewest expected word (character) errors against the other rows, those weighted
        by exp(mbr_scale * score), comes first.  qasr_ctc_mbr runs behind the beam chain on the same stream over the beam's
        buffers as they lie (the NumPy twin for CPU tensors and the host modules); the lists come back in MBR order and
        every hypothesis carries posterior, mbr_risk (its expected errors) and beam_rank (its place in the beam's list).
        mbr_scale: 0 .. 16; 1.0 is a starting point, not a tuned value.  timestamps / posteriors align the rows as they lie;
        the lists are re-ordered afterwards.  lm, boost and sample_rate compose unchanged.

        sample_rate / channels: as for forward() - PCM at another rate is resampled first; times stay seconds."""
        from qasr import ctc as qctc
        mbr = self._mbr_args('decode', mbr, mbr_scale, beam_width, n_best)                            # refused before anything runs
        input_signal, input_signal_length = self._resample_in(input_signal, input_signal_length, sample_rate, channels)
        if lm is not None and beam_width is None:
            raise ValueError('decode: lm needs beam_width (the greedy collapse has no language model)')
        if boost is not None and beam_width is None:
            raise ValueError('decode: boost needs beam_width (the greedy collapse has no phrase boosting)')
        if posteriors and beam_width is None:
            raise ValueError('decode: posteriors needs beam_width (greedy hypotheses are not aligned against a text)')
        if posteriors and not timestamps:
            raise ValueError('decode: posteriors needs timestamps=True (the posteriors are those of the alignment)')
        if beam_width is not None:
            beam_width, n_best, cutoff_top_n = self._beam_args(beam_width, n_best, cutoff_top_n)      # refused before any launch
            lm = self._lm_args(lm, alpha, beta)
            if boost is not None:
                from qasr import boost as qboost
                try:
                    boost = qboost.as_phrase_set(boost, self.decoder.vocabulary, boost_weight)
                except ValueError as e:
                    raise ValueError(f'decode: {e}') from None
            return self._beam_decode(self._forward(input_signal, input_signal_length, processed_signal, processed_signal_length),
                                     beam_width, n_best, cutoff_top_n, lm, alpha, beta, bool(timestamps), boost, bool(posteriors),
                                     rows=_rows, mbr=mbr)
        res = self._forward(input_signal, input_signal_length, processed_signal, processed_signal_length, decode=True)
        if _rows:                            # error_rate: the CtcResult as it lies, nothing turned into strings
            return res
        return qctc.to_hypotheses(res, self.decoder.vocabulary, self.seconds_per_frame())

    def _long_plan(self, lens_samples, window_s=30.0, overlap_s=4.0, guard_s=1.0):
        """the qasr.longform.WindowPlan of decode_long for recordings of lens_samples samples at the model's rate; its row
        pitch counts the frames the front-end pads a window to (pad_to), as the engine's outputs do"""
        from qasr import longform as qlong, ragged
        f = self.preprocessor.featurizer
        rate = int(self.preprocessor._sample_rate)
        spf = int(round(self.seconds_per_frame() * rate))
        stride = max(spf // int(f.hop_length), 1)
        pad_to = int(f.pad_to) if isinstance(f.pad_to, int) and f.pad_to > 0 else 0

        def frames_of(n):
            t = 1 + n // int(f.hop_length)
            if pad_to and t % pad_to:
                t += pad_to - t % pad_to
            return -(-t // stride)

        return qlong.WindowPlan(lens_samples, window_s, overlap_s, guard_s, rate, spf, frames_of)

    def _long_windows(self, plan, windows, wlens, len_dtype, batch_size, want, cutoff_top_n=None):
        """The windows of a plan through the model in batches of batch_size (decode_long, align_long): tokens int32
        [Wn, Tw], frame scores float32 [Wn, Tw], encoded lengths int32 [Wn] and the extra planes of `want` - 'frames': none
        (on the static engine no log-probability tensor is written); 'topn': the cutoff_top_n candidates per frame (ids,
        q), the log-probabilities living for one batch; 'logp': the log-probabilities themselves, float32 [Wn, Tw, C].  On
        the calibrated model without a reservation, (batch_size, window) is reserved for the duration of the call."""
        from qasr import beam as qbeam, engine as qengine
        cuda = windows.is_cuda
        own = cuda and self._reserve is None and self.engine_ready()
        if own:                              # for this call: every full batch replays one graph
            self._reserve = (batch_size, max(plan.Wl, windows.shape[1]) / float(plan.sample_rate))
            self._reserve_logp = want != 'frames'
        toks = fs = enc = None
        extra = []
        try:
            for i in range(0, plan.Wn, batch_size):
                sig, ln = windows[i:i + batch_size], wlens[i:i + batch_size].to(len_dtype)
                if want == 'frames':
                    t, f, e = self._forward(sig, ln, decode='frames')
                    c = ()
                else:                        # the log-probabilities live for one batch: only the candidates are kept
                    logp, e, t = self._forward(sig, ln)
                    f = self._frame_scores(logp, t)
                    if want == 'logp':
                        c = (logp.float(),)
                    elif cuda:
                        c = qengine.ctc_topn(logp.float(), e, cutoff_top_n)
                    else:
                        c = [torch.from_numpy(x) for x in qbeam.topn_host(logp.float().numpy(), cutoff_top_n, e.numpy())]
                if toks is None:
                    Tw, dev = t.shape[1], t.device
                    toks = torch.empty(plan.Wn, Tw, device=dev, dtype=torch.int32)
                    fs = torch.empty(plan.Wn, Tw, device=dev, dtype=torch.float32)
                    enc = torch.empty(plan.Wn, device=dev, dtype=torch.int32)
                    extra = [torch.empty((plan.Wn, Tw) + tuple(x.shape[2:]), device=dev, dtype=x.dtype) for x in c]
                b = t.shape[0]
                toks[i:i + b].copy_(t)
                fs[i:i + b].copy_(f)
                enc[i:i + b].copy_(e)
                for dst, x in zip(extra, c):
                    dst[i:i + b].copy_(x)
        finally:
            if own:
                self._reserve, self._reserve_logp = None, True
        return toks, fs, enc, tuple(extra)

    @torch.no_grad()
    def decode_long(self, input_signal, input_signal_length, window_s=30.0, overlap_s=4.0, guard_s=1.0, batch_size=32,
                    seam='blank', beam_width=None, n_best=1, cutoff_top_n=40, lm=None, alpha=0.0, beta=0.0, boost=None,
                    boost_weight=1.0, sample_rate=None, channels=1, _rows=False, mbr=None):
        """Hypotheses of long recordings (an extension; buffered inference on the device): input_signal [R, S] with
        input_signal_length samples each -> List[qasr.ctc.Hypothesis], one per recording, times in seconds of the recording,
        seams_s = the times at which neighbouring windows were joined (None for a recording of one window: its hypothesis
        is decode()'s).

        Each recording is cut into windows of window_s seconds that overlap by overlap_s (k_cut); the windows of all
        recordings run through the model in batches of batch_size - on the calibrated model through a reserved engine, so
        every batch replays one captured graph: reserve() is honoured, and without one (batch_size, window_s) is reserved
        for the duration of the call - then k_stitch joins the windows' frames at one seam per pair, chosen under
        qasr.longform.SEAM_RULES (seam='blank': where both windows agree on a blank, the most confident such frame, then
        the middle of the overlap; 'middle': the middle alone), keeping guard_s of every window edge out of the choice, and
        the greedy collapse (k_ctc) runs once on the stitched rows.  The greedy path keeps tokens and per-frame scores only:
        on the static engine no log-probability tensor is written.  beam_width / n_best / cutoff_top_n / lm / alpha / beta /
        boost / boost_weight: as decode(); k_topn runs per batch, the candidates are stitched and the beam search runs once
        per recording, which may then have at most qasr.beam.MAX_T (QASR_BEAM_MAX_FRAMES) stitched frames; beam hypotheses
        carry no times.  sample_rate / channels: as forward().  CPU inputs run the NumPy twins.  When no recording of the
        batch is longer than a window, nothing is cut and the batch runs as decode() runs it: the hypotheses are decode()'s.

        Normalisation - the front-end's per-feature statistics, dynamic ranges - is per window: the result is NOT that of
        decode() over the whole recording, and the defaults (30 s / 4 s / 1 s) are not tuned on speech."""
        from qasr import beam as qbeam, ctc as qctc, engine as qengine
        if input_signal is None or input_signal_length is None:
            raise ValueError('decode_long: input_signal and input_signal_length are required')
        if mbr is not None:
            raise ValueError('decode_long: mbr is not built for long recordings (stitched rows make the pair workspace a separate '
                             'question; see "Minimum Bayes risk re-ranking" in the README): re-rank decode()\'s lists, or '
                             'qasr.mbr.rerank_texts over the texts')
        if lm is not None and beam_width is None:
            raise ValueError('decode_long: lm needs beam_width (the greedy collapse has no language model)')
        if boost is not None and beam_width is None:
            raise ValueError('decode_long: boost needs beam_width (the greedy collapse has no phrase boosting)')
        if seam not in ('blank', 'middle'):
            raise ValueError(f"decode_long: seam must be 'blank' or 'middle', got {seam!r}")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f'decode_long: batch_size must be at least 1, got {batch_size}')
        if beam_width is not None:
            beam_width, n_best, cutoff_top_n = self._beam_args(beam_width, n_best, cutoff_top_n)
            lm = self._lm_args(lm, alpha, beta)
            if boost is not None:
                from qasr import boost as qboost
                try:
                    boost = qboost.as_phrase_set(boost, self.decoder.vocabulary, boost_weight)
                except ValueError as e:
                    raise ValueError(f'decode_long: {e}') from None
        signal, length = self._resample_in(input_signal, input_signal_length, sample_rate, channels)
        if signal.dim() != 2:
            raise ValueError(f'decode_long: input_signal must be [R, S], got {tuple(signal.shape)}')
        signal = signal.float()
        lens_host = length.detach().cpu().long().clamp(max=signal.shape[1])
        plan = self._long_plan(lens_host.numpy(), window_s, overlap_s, guard_s)      # refuses its arguments by name
        blank = len(self.decoder.vocabulary)
        cuda = signal.is_cuda
        if plan.Wn == plan.R:                # nothing to cut: the batch runs as decode() runs it, padded as it came (the
            windows, wlens = signal, lens_host.to(signal.device)      # front-end's reflect padding folds at the batch's width)
        else:
            windows, wlens = qengine.longform_cut(signal, lens_host.to(signal.device), plan)
        toks, fs, enc, planes = self._long_windows(plan, windows, wlens, length.dtype, batch_size,
                                                   'frames' if beam_width is None else 'topn', cutoff_top_n)
        out, total, seams = qengine.longform_stitch(plan, enc, toks, fs, planes, blank, seam)
        spf_s = self.seconds_per_frame()
        seams_h = seams.cpu().numpy()
        seams_s = [[float(seams_h[w]) * spf_s for w in range(int(plan.first[r]) + 1, int(plan.first[r]) + int(plan.count[r]))]
                   if plan.count[r] > 1 else None for r in range(plan.R)]      # one window: decode()'s own hypothesis
        if beam_width is None:
            if cuda:
                res = qengine.ctc_collapse(out[0], out[1], total, blank=blank)
            else:
                res = qctc.collapse_host(out[0].numpy(), out[1].numpy(), total.numpy(), blank=blank)
            if _rows:                        # error_rate_long: the stitched rows' CtcResult as it lies
                return res
            hyps = qctc.to_hypotheses(res, self.decoder.vocabulary, spf_s)
            for h, s in zip(hyps, seams_s):
                h.seams_s = s
            return hyps
        total_h = total.cpu().numpy()
        for r in range(plan.R):
            if int(total_h[r]) > qbeam.MAX_T:
                raise ValueError(f'decode_long: recording {r} has {int(total_h[r])} stitched frames; the beam search takes at most '
                                 f'QASR_BEAM_MAX_FRAMES = {qbeam.MAX_T} frames per recording')
        T = max(int(total_h.max()), 1)
        scid, scq = out[2][:, :T].contiguous(), out[3][:, :T].contiguous()
        if cuda:
            res = qengine.ctc_beam(scid, scq, total, blank, beam_width, n_best, lm=lm, alpha=alpha, beta=beta, boost=boost)
        else:
            res = qbeam.beam_search_host(scid.numpy(), scq.numpy(), total_h, blank, beam_width, n_best, lm, alpha, beta, boost)
        if _rows:
            return res
        hyps = qbeam.to_hypotheses(res, self.decoder.vocabulary)
        for row, s in zip(hyps, seams_s):
            for h in row:
                h.seams_s = s
        return hyps if n_best > 1 else [h[0] for h in hyps]

    def _reference_rows(self, who, targets, target_lengths, texts, n, device):
        """the references of error_rate as (ids [n, L], lengths [n] or None) on `device`: targets / target_lengths as the data
        loader gives them (no lengths: the padded rows), or texts over the decoder's vocabulary of single characters"""
        if (targets is None) == (texts is None):
            raise ValueError(f'{who}: give the references as targets (with target_lengths) or as texts, not both')
        if texts is not None:
            at = {ch: i for i, ch in enumerate(self.decoder.vocabulary)}
            if len(texts) != n:
                raise ValueError(f'{who}: {len(texts)} texts for {n} utterances')
            ids = []
            for r, t in enumerate(texts):
                for ch in t:
                    if ch not in at:
                        raise ValueError(f'{who}: text {r} has {ch!r}, which is not in the vocabulary')
                ids.append([at[ch] for ch in t])
            targets = torch.zeros(n, max(1, max(len(x) for x in ids)), dtype=torch.int32)
            for r, x in enumerate(ids):
                targets[r, :len(x)] = torch.tensor(x, dtype=torch.int32)
            target_lengths = torch.tensor([len(x) for x in ids], dtype=torch.int32)
        if targets.dim() != 2 or targets.shape[0] != n:
            raise ValueError(f'{who}: targets must be [{n}, ids], got {tuple(targets.shape)}')
        if targets.shape[1] == 0:
            targets, target_lengths = torch.zeros(n, 1, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
        return targets.to(device), None if target_lengths is None else target_lengths.to(device)

    def _score_rows(self, who, res, targets, target_lengths, texts, use_cer, alignments=False, max_workspace_bytes=1 << 30):
        """error_rate behind any decode chain: the CtcResult's or BeamResult's label rows against the references through k_edit
        (cuda) or its twin; only the counts are read back.  alignments: the best rows (k = 0) also go through k_edit_trace or
        its twin, and ops, n_ops and the label rows are read back for the report's Alignments"""
        from qasr import edit as qedit
        vocab = self.decoder.vocabulary
        labels, n_labels = res.labels, res.n_labels
        n_hyps = getattr(res, 'n_hyps', None)
        K = labels.shape[1] if n_hyps is not None else 1
        cuda = torch.is_tensor(labels) and labels.is_cuda
        n = labels.shape[0]
        hyp, hl = labels.reshape(n * K, labels.shape[-1]), n_labels.reshape(n * K)
        tg, tl = self._reference_rows(who, targets, target_lengths, texts, n, labels.device if cuda else 'cpu')
        mode = 'char' if use_cer else 'word'
        mask = None if use_cer else qedit.space_mask(list(vocab), who)
        if cuda:
            sp = None if mask is None else torch.from_numpy(mask).to(labels.device)
            out = qedit.edit_device(hyp, hl, tg, tl, len(vocab), mode=mode, is_space=sp, rows_per_ref=K, n_hyps=n_hyps)
            rows, totals = out.rows.cpu().numpy(), out.totals.cpu().numpy()
        else:
            host = lambda t: None if t is None else (t.numpy() if torch.is_tensor(t) else t)
            out = qedit.edit_host(host(hyp), host(hl), host(tg), host(tl), len(vocab), mode=mode, is_space=mask, rows_per_ref=K,
                                  n_hyps=host(n_hyps))
            rows, totals = out.rows, out.totals
        rep = qedit.report_of(rows, totals, K)
        mres = getattr(res, 'mbr', None)
        if mres is not None:                 # the counts of the MBR picks: the rows read back above, and order[:, 0]
            pick = mres.order[:, 0]
            pick = (pick.cpu().numpy() if torch.is_tensor(pick) else np.asarray(pick)).astype(np.int64)
            r = np.asarray(rows).reshape(n, K, -1)[np.arange(n), np.maximum(pick, 0)].astype(np.int64)
            r = r[(pick >= 0) & (r[:, 6] == 1)]
            rep.mbr_total = qedit.counts_of(*(int(r[:, c].sum()) for c in (0, 1, 2, 3, 4, 5)))
            rep.mbr_pick = pick.tolist()
        if alignments:
            hyp0, hl0 = (hyp, hl) if K == 1 else (labels[:, 0], n_labels[:, 0])          # the k = 0 rows, where they lie
            n0 = None if n_hyps is None else (n_hyps.clamp(max=1) if torch.is_tensor(n_hyps) else np.minimum(n_hyps, 1))
            if cuda:
                tr = qedit.trace_device(hyp0, hl0, tg, tl, len(vocab), mode=mode, is_space=sp, n_hyps=n0,
                                        max_workspace_bytes=max_workspace_bytes)
                cpu = lambda t: None if t is None else t.cpu().numpy()
                tr = qedit.TraceResult(rows.reshape(n, K, -1)[:, 0], cpu(tr.ops), cpu(tr.n_ops), 1)    # the rows are k_edit's
            else:
                cpu = host
                tr = qedit.trace_host(cpu(hyp0), cpu(hl0), cpu(tg), cpu(tl), len(vocab), mode=mode, is_space=mask, n_hyps=cpu(n0),
                                      max_workspace_bytes=max_workspace_bytes)
            rep.alignments = qedit.alignments_of(tr, cpu(hyp0), cpu(hl0), cpu(tg), cpu(tl), list(vocab), mode=mode, is_space=mask)
        return rep

    @torch.no_grad()
    def error_rate(self, input_signal=None, input_signal_length=None, targets=None, target_lengths=None, texts=None, use_cer=False,
                   beam_width=None, n_best=1, processed_signal=None, processed_signal_length=None, alignments=False,
                   max_workspace_bytes=1 << 30, **decode_args):
        """Word (use_cer: character) error counts of one batch against its references (an extension): decode()'s device
        chain - greedy, or the beam search with beam_width / n_best and decode()'s cutoff_top_n, lm, alpha, beta, boost,
        boost_weight, sample_rate, channels - then the edit distance over the label rows where they lie (k_edit;
        qasr.edit.EDIT_RULES).  Only the counts are read back: a qasr.ctc.ErrorReport with the total over the best
        hypotheses, the per-utterance counts and, with n_best = K > 1, oracle_errors = the sum over the utterances of the
        fewest errors among their K rows.  References: targets int [B, L] with target_lengths (None: the padded rows), or
        texts.  The numbers are word_error_rate's over decode()'s texts.  Works on the static engine, a reserved engine, the
        dynamic path, and through the NumPy twin with the host modules or CPU tensors.  Word mode needs a vocabulary of
        single characters.  alignments=True: the report also carries one qasr.ctc.Alignment per utterance for its best row
        (k_edit_trace, qasr.edit.TRACE_RULES; ops, n_ops and the label rows are read back); a batch whose back-pointer plane
        would exceed max_workspace_bytes is refused by name.  mbr='word' | 'char' with mbr_scale, as decode() takes them: the
        report also carries mbr_total, the counts of every utterance's MBR pick (qasr.mbr.MBR_RULES), and mbr_pick - so one call
        tells how wrong the first row is (total), the reference-free pick (mbr_total) and the best row of the list
        (oracle_errors)."""
        for k in ('timestamps', 'posteriors', '_rows'):
            if k in decode_args:
                raise ValueError(f'error_rate: {k} is not an argument of the error rate')
        res = self.decode(input_signal, input_signal_length, processed_signal, processed_signal_length, beam_width=beam_width,
                          n_best=n_best, _rows=True, **decode_args)
        return self._score_rows('error_rate', res, targets, target_lengths, texts, use_cer, bool(alignments), max_workspace_bytes)

    @torch.no_grad()
    def error_rate_long(self, input_signal, input_signal_length, targets=None, target_lengths=None, texts=None, use_cer=False,
                        beam_width=None, n_best=1, alignments=False, max_workspace_bytes=1 << 30, **decode_long_args):
        """error_rate behind decode_long's stitched rows: window_s / overlap_s / guard_s / batch_size / seam and the beam
        arguments as decode_long takes them, one reference per recording; alignments / max_workspace_bytes as error_rate's."""
        if '_rows' in decode_long_args:
            raise ValueError('error_rate_long: _rows is not an argument of the error rate')
        res = self.decode_long(input_signal, input_signal_length, beam_width=beam_width, n_best=n_best, _rows=True,
                               **decode_long_args)
        return self._score_rows('error_rate_long', res, targets, target_lengths, texts, use_cer, bool(alignments),
                                max_workspace_bytes)

    def _stream_plan(self, chunk_s=0.96, left_s=4.0, right_s=0.96):
        """the qasr.stream.StreamPlan of stream(): units and frames_of taken from the model as _long_plan takes them"""
        from qasr import stream as qstream
        lp = self._long_plan([1])
        return qstream.StreamPlan(chunk_s, left_s, right_s, lp.sample_rate, lp.samples_per_frame, lp.frames_of)

    def stream(self, max_streams=32, chunk_s=0.96, left_s=4.0, right_s=0.96, tail=True, sample_rate=None, beam_width=None,
               input_rate=None, channels=1, beam=None, boost=None, endpoint=None, spot=None):
        """A streaming session (an extension; NeMo's buffered streaming, the FrameBatchASR idea, for many streams at once):

            sess = model.stream(max_streams=32, chunk_s=0.96, left_s=4.0, right_s=0.96)
            slot = sess.open()
            updates = sess.push(slots, signal[B, n], lengths)      # any n; float32 or int16 at the model's rate
            hyp = sess.close(slot)                                  # the END step; the slot is free again

        The models are not causal and normalise per utterance, so nothing is cached: whenever a stream has received another
        chunk_s seconds, a step runs the window [left_s of context | the chunk | right_s of look-ahead] of its latest
        samples through the model - the same _forward call decode_long makes, so the static engine, a reserved engine, the
        dynamic path and the host modules all work - and the chunk's frames become final, right_s late (qasr.stream.
        STREAM_RULES).  The samples, the counters, the open run and the score sums of every stream stay on the device
        (k_stream_push, k_stream_window, k_stream_emit); a step reads back its small delta only.  push() returns one
        qasr.ctc.StreamUpdate per step and stream; close() returns the qasr.ctc.Hypothesis of the whole stream (text, label
        and word times, confidences, utt_score), equal on every byte to the greedy collapse of the final frames.  tail=True
        also lists the provisional text of the look-ahead frames.  CPU tensors run the NumPy twins.

        On the calibrated model the session holds a reservation of (max_streams, window) for its lifetime - every step of
        full windows replays one captured graph and the engine allocates nothing (its device_allocs counter stands still;
        the session's small uploads of slots / flags / counts and its chunk staging go through torch's caching allocator) -
        and close_all() / leaving the `with` block restores the caller's.  Results do not depend on how the caller slices its pushes.  On the static engine a
        stream's result does not depend on which other streams shared its steps either; on the dynamic path the ranges
        are derived per batch, so there it does.

        Normalisation is per window; the first left_s seconds of a stream see less context; the latency is chunk_s +
        right_s plus the step; the defaults are untried on speech.

        input_rate=R, channels=C: the streams carry PCM at R Hz - int16 or float32, C interleaved channels (1 .. 8) - as
        push(slots, signal[B, n * C], lengths in frames).  Every stream keeps its own resampler state on the device next
        to its ring (k_stream_rs_append, k_stream_rs_fir; qasr.stream_rs states the rule): the filter is
        model.resample_quality's, a slot keeps the sample format of its first push, and however the pushes are sliced
        the samples that reach the stream's ring are qasr.resample.resample_host of the whole stream on every byte - so
        the session gives what a session at the model's rate gives for the offline resampler's output.  Times stay seconds
        of the stream (frames are counted at the model's rate).  A resampled sample is final once the W input frames
        behind it have arrived, so the filter adds W / R seconds of latency (8.5 ms at 8 kHz 'best', 4.2 ms at 48 kHz
        'best'); close() flushes that tail, and the updates of steps it completes are kept in sess.closing_updates.
        input_rate=None, or the model's rate with channels=1, is the plain session.

        beam=qasr.stream_beam.StreamBeam(width=16, n_best=1, cutoff_top_n=40, lm=None, alpha=0.0, beta=0.0, lag_s=4.0): the
        prefix beam search of decode(beam_width=, lm=) across steps.  Every stream keeps its beam on the device next to its
        ring (k_stream_beam; qasr.stream_beam.STREAM_BEAM_RULES states the rule); a step is window -> forward with
        log-probabilities -> top-N -> beam -> emit.  Text becomes final by a fixed-lag commit: every 32 frames the labels of
        the best entry created more than lag_s ago are committed and entries that disagree with them are dropped, keyed on
        the global frame, so the result does not depend on how the pushes are sliced.  push() then returns StreamUpdates
        whose labels / text are the newly committed labels, start_s / end_s the frame at which each label entered the beam
        (a free emission time, not an alignment), score empty (a committed prefix has no score of its own) and tail_text
        the best entry's uncommitted text; close() returns the Hypothesis of committed text + the best remainder with
        utt_score = the beam score and lm_score, or with n_best > 1 the list, best first, as decode(beam_width=, n_best=)
        returns it.  lag_s beyond the stream's length gives decode(beam_width=)'s result for the final frames.  The
        default lag of 4.0 s is untried on speech.  It composes with input_rate= unchanged: everything here sits behind
        the ring.

        StreamBeam(..., boost=, boost_weight=1.0): phrase boosting across steps (qasr.stream_beam.STREAM_BOOST_RULES;
        k_stream_beam_boost keeps every beam entry's automaton state and running bonus in the slot's block).  boost is a
        list of phrases as decode(boost=) takes it, a qasr.boost.PhraseSet, or a dict of at most 8 named sets; the sets are
        compiled against the vocabulary, packed, checked and uploaded once, here.  With one set every stream uses it and
        sess.open(boost=False) opts a stream out; with a dict sess.open(boost='name') picks a set and None means the
        stream is not boosted.  close() fills boost_score as decode(boost=) does; utt_score includes it, lm_score does
        not.  A session without boost allocates, launches and stores exactly what it did.

        endpoint=qasr.stream_ep.Endpointing(silence_s=0.8, start_timeout_s=5.0, max_utt_s=30.0, hard_max_s=40.0,
        min_logp=None): the stream is cut into utterances on the device (k_stream_endpoint behind k_stream_emit in every
        step; qasr.stream_ep.EP_RULES states the rule).  It is decoder-driven - a final frame is speech when its arg-max is
        not blank (and its score is at least min_logp) - with Kaldi-style integer rules over global frames: silence_s
        without speech after speech, start_timeout_s without any speech, max_utt_s (cut at the next blank frame),
        hard_max_s (cut wherever it stands; a run that spans the cut goes to the next utterance).  push() returns the same
        StreamUpdates; finished utterances queue up in sess.take_utterances() as qasr.ctc.StreamUtterance(slot, index,
        reason, start_s, end_s, speech_start_s, speech_end_s, hypothesis) - 'timeout' utterances are delivered too, with no
        text when min_logp is unset - and the host keeps the deltas of the open utterance only.  close() returns the
        Hypothesis of the last ('end') utterance and queues it as well.  The results do not depend on how the pushes are
        sliced.  All five defaults are untried on speech.  It composes with input_rate= unchanged.

        StreamBeam(..., endpoint=Endpointing(...)): endpointing in a beam session (qasr.stream_beam.STREAM_BEAM_EP_RULES;
        k_stream_beam_ep).  A step is window -> forward with log-probabilities -> top-N -> emit -> endpoint -> beam: the cuts are
        decided by the greedy arg-max as above, and at every cut the slot's beam is finalised as at END and reset to the single
        fresh entry (LM context and boost state at their starts; the slot's phrase set stays).  push() returns the beam
        session's StreamUpdates (tail_text behind a cut is the fresh beam's); take_utterances() delivers StreamUtterances whose
        span, speech span and reason come from the record and whose hypothesis is the BEAM's best for that utterance - text,
        labels, creation-frame times in seconds of the stream, utt_score / lm_score / boost_score of that utterance alone -
        and with n_best > 1 StreamUtterance.n_best carries the list.  close() returns the 'end' utterance's hypothesis (the
        list with n_best > 1).  A 'hard' cut can split a label's frames, so the label can show up at the end of one utterance
        and at the start of the next; a 'timeout' utterance reports whatever the beam holds, normally nothing.

        spot=qasr.stream_spot.StreamSpot(keywords=[...], labels=None, threshold=-1.0, max_span_s=10.0): keyword spotting on the
        live stream (qasr.stream_spot.STREAM_SPOT_RULES; k_star with penalty 0 and k_stream_spot behind k_stream_emit in every
        step).  The keywords are spot()'s - the same parser, the same refusals - and are shared by all streams of the session;
        every (stream, keyword) keeps its lattice row and one open hit on the device next to the stream state, and the session
        forwards with log-probabilities.  push() returns the same StreamUpdates and close() what it returned; the hits that
        closed - the END step's included - queue up in sess.take_hits() as qasr.ctc.StreamHit(slot, hit, detected_s), hit a
        qasr.ctc.KeywordHit in seconds of the stream, sorted by (detected_s, slot, start_s, index); sess.pending_hits(slot)
        lists the hits that are open after the last step: the provisional, immediate detection, which a later frame may still
        replace by an overlapping hit with a higher mean.  The final hits of a stream are spot()'s hits over its final frames
        on every byte, however the pushes are sliced.  A hit becomes final only when nothing can overlap it any more: on
        blank-dominated audio that is up to max_span_s after its end, so a wake-word caller sets max_span_s near the keyword's
        longest plausible duration and acts on pending_hits.  Both defaults are untried on speech.  It composes with
        input_rate= and endpoint= unchanged; spot= together with beam= is not built.

        Refused: sample_rate other than the model's (here it names the model's rate: give the source's as input_rate=),
        a rate or filter the resampler refuses, channels outside 1 .. 8, beam_width (beam search across steps is beam=),
        boost (phrase boosting across steps is StreamBeam(boost=)), beam= arguments outside decode(beam_width=)'s ranges,
        more than 8 phrase sets or an empty dict of them, a set that qasr.boost.PhraseSet refuses, boost_weight outside
        0 .. 16, endpoint= times the plan refuses, beam= together with endpoint= (the endpointing of a beam session is
        StreamBeam(endpoint=)), spot= that is no StreamSpot, whatever spot() refuses about its keywords, threshold and
        max_span_s, spot= together with beam=."""
        target = int(self.preprocessor._sample_rate)
        if sample_rate is not None and int(sample_rate) != target:
            raise ValueError(f'stream: sample_rate {sample_rate} is not the model\'s {target}: sample_rate names the model\'s rate '
                             'here; give the rate of the audio as input_rate=')
        if beam_width is not None:
            raise ValueError('stream: beam_width is not an argument of stream(): give the streaming beam search as '
                             'beam=qasr.stream_beam.StreamBeam(width=...)')
        if boost is not None:
            raise ValueError('stream: boost is not an argument of stream(): give the phrases of the streaming beam search as '
                             'beam=qasr.stream_beam.StreamBeam(boost=...)')
        if int(max_streams) < 1:
            raise ValueError(f'stream: max_streams must be at least 1, got {max_streams}')
        try:
            plan = self._stream_plan(chunk_s, left_s, right_s)
        except ValueError as e:
            raise ValueError(f'stream: {e}') from None
        from qasr import resample as qresample, stream_rs as qsrs
        if not 1 <= int(channels) <= qresample.MAX_CHANNELS:
            raise ValueError(f'stream: channels must be 1 .. {qresample.MAX_CHANNELS}, got {channels}')
        if input_rate is None and int(channels) != 1:
            raise ValueError('stream: channels needs input_rate (the rate of the interleaved PCM)')
        rs_plan = None
        if input_rate is not None and not (int(input_rate) == input_rate and int(input_rate) == target and int(channels) == 1):
            key = (int(input_rate) if int(input_rate) == input_rate else input_rate, target, self.resample_quality)
            plans = self.__dict__.setdefault('_resample_plans', {})
            try:
                if key not in plans:
                    plans[key] = qresample.ResamplePlan(input_rate, target, self.resample_quality)
                rs_plan = qsrs.StreamResamplePlan(plan, plans[key], int(channels))
            except ValueError as e:
                raise ValueError(f'stream: input_rate {input_rate}: {e}') from None
        sspot = None
        if spot is not None:
            from qasr import spot as qspot, stream_spot as qss
            if not isinstance(spot, qss.StreamSpot):
                raise ValueError(f'stream: spot must be a qasr.stream_spot.StreamSpot, got {type(spot).__name__}')
            if beam is not None:
                raise ValueError('stream: spot= together with beam= is not built: keyword spotting runs in sessions of the greedy '
                                 'decoder (with or without endpoint=)')
            given, tg, tl, thr, span, _ = self._spot_args('stream: spot', spot.keywords, spot.labels, spot.threshold, spot.max_span_s, 1)
            sspot = (spot, given, qss.StreamSpotPlan(plan, tg, tl, qspot.check_threshold(thr, 'stream: spot'), span))
        bplan = None
        if beam is not None:
            from qasr import stream_beam as qsb
            if not isinstance(beam, qsb.StreamBeam):
                raise ValueError(f'stream: beam must be a qasr.stream_beam.StreamBeam, got {type(beam).__name__}')
            try:
                w, nb, n = self._beam_args(beam.width, beam.n_best, beam.cutoff_top_n)
                lm = self._lm_args(beam.lm, beam.alpha, beam.beta)
                sets, bw = self._stream_boost_sets(beam.boost, beam.boost_weight)
                beam = qsb.StreamBeam(w, nb, n, lm, float(beam.alpha), float(beam.beta), beam.lag_s, sets, bw, beam.endpoint)
                bplan = qsb.StreamBeamPlan.for_stream(plan, beam)
            except ValueError as e:
                raise ValueError('stream: beam: ' + str(e).replace('decode: ', '')) from None
        eplan = None
        if beam is not None and beam.endpoint is not None:
            from qasr import stream_ep as qse
            if endpoint is not None:
                raise ValueError('stream: beam= together with endpoint= is not supported: the session already cuts by '
                                 'StreamBeam(endpoint=), which finalises and resets the beam at a cut')
            if not isinstance(beam.endpoint, qse.Endpointing):
                raise ValueError(f'stream: beam: endpoint must be a qasr.stream_ep.Endpointing, got {type(beam.endpoint).__name__}')
            try:
                eplan = qse.EndpointPlan.for_stream(plan, beam.endpoint)
            except ValueError as e:
                raise ValueError(f'stream: beam: endpoint: {e}') from None
            return StreamSession(self, int(max_streams), plan, bool(tail), rs_plan, beam, bplan, beam.endpoint, eplan)
        if endpoint is not None:
            from qasr import stream_ep as qse
            if not isinstance(endpoint, qse.Endpointing):
                raise ValueError(f'stream: endpoint must be a qasr.stream_ep.Endpointing, got {type(endpoint).__name__}')
            if beam is not None:
                raise ValueError('stream: beam= together with endpoint= is not supported: give the endpointing of a beam session as '
                                 'beam=qasr.stream_beam.StreamBeam(endpoint=...), which finalises and resets the beam at a cut')
            try:
                eplan = qse.EndpointPlan.for_stream(plan, endpoint)
            except ValueError as e:
                raise ValueError(f'stream: endpoint: {e}') from None
        return StreamSession(self, int(max_streams), plan, bool(tail), rs_plan, beam, bplan, endpoint, eplan, sspot)

    @torch.no_grad()
    def decode_stream(self, input_signal, input_signal_length, chunk_s=0.96, left_s=4.0, right_s=0.96, session=None, input_rate=None,
                      channels=1, beam=None, endpoint=None, spot=None):
        """A batch of complete recordings played through a streaming session, all rows side by side in pushes of chunk_s
        seconds (what inference.py --stream_chunk_s does): List[qasr.ctc.Hypothesis], one per row - the hypotheses
        stream() gives for that audio, which do not depend on the size of the pushes.

        session=<a session of this model with at least B free slots> plays the batch through it and leaves it open.
        Without one, a session is opened and closed per call - and on the calibrated model that is not free: taking and
        restoring the reservation closes the reserved engine each time (a caller's own included), so the engine is built
        and its graph captured again for every call.  A caller with many batches holds one session across them.

        input_rate=R, channels=C: the recordings are PCM at R Hz, [B, S * C] interleaved, lengths in frames, as for
        stream(); a session passed in carries its own.  beam=: the streaming beam search of stream(beam=); the rows are then
        what close() returns there (a list per row with n_best > 1); with StreamBeam(endpoint=) the rows are the recordings'
        utterances, as with endpoint=.  endpoint=: the endpointing of stream(endpoint=); the
        rows are then lists of qasr.ctc.StreamUtterance, every utterance of the recording in order (utterances that were
        waiting in a passed session's queue before the call are left there).  spot=: the keyword spotting of stream(spot=); the
        call then returns the pair (the rows as above, one list of qasr.ctc.KeywordHit per recording: its final hits in the
        order of take_hits - sess.decoded_hits keeps them as StreamHits, with detected_s, until the next call); hits that were
        waiting in a passed session's queue are left there."""
        ch = session.rs_plan.channels if session is not None and session.rs_plan is not None else int(channels)
        if input_signal.dim() != 2 or ch < 1 or input_signal.shape[1] % ch:
            raise ValueError(f'decode_stream: input_signal must be [B, S * channels], got {tuple(input_signal.shape)} for {channels} channels')
        B = input_signal.shape[0]
        lens = [min(int(n), input_signal.shape[1] // ch) for n in input_signal_length.tolist()]
        sess = session if session is not None else self.stream(max_streams=B, chunk_s=chunk_s, left_s=left_s, right_s=right_s, tail=False,
                                                               input_rate=input_rate, channels=ch, beam=beam, endpoint=endpoint, spot=spot)
        try:
            waiting = sess.take_utterances() if sess.endpoint is not None else []
            waiting_hits = sess.take_hits() if sess.spot is not None else []
            slots = [sess.open() for _ in range(B)]
            C = sess.plan.C if sess.rs_plan is None else sess.rs_plan.Ain     # about chunk_s of audio per push
            for off in range(0, max(lens + [0]), C):
                live = [b for b in range(B) if off < lens[b]]
                sess.push([slots[b] for b in live], input_signal[live, off * ch:(off + C) * ch], [min(C, lens[b] - off) for b in live])
            hyps = [sess.close(s) for s in slots]
            if sess.endpoint is not None:
                utts = sess.take_utterances()
                sess._utts = waiting
                hyps = [[u for u in utts if u.slot == s] for s in slots]
            if sess.spot is None:
                return hyps
            hits = sess.take_hits()
            sess._hits = waiting_hits
            sess.decoded_hits = [[h for h in hits if h.slot == s] for s in slots]      # the same with their detection times
            return hyps, [[h.hit for h in row] for row in sess.decoded_hits]
        finally:
            if session is None:
                sess.close_all()

    def _stream_boost_sets(self, boost, boost_weight):
        """StreamBeam(boost=, boost_weight=) -> (None | {name: qasr.boost.PhraseSet}, weight): a single set goes under the
        name None; every set is compiled against the model's vocabulary here, before anything is launched"""
        from qasr import boost as qboost, stream_beam as qsb
        w = float(boost_weight)
        if not 0.0 <= w <= qboost.MAX_WEIGHT:                # (NaN fails both comparisons)
            raise ValueError(f'boost_weight must be 0 .. {qboost.MAX_WEIGHT:g}, got {boost_weight}')
        if boost is None:
            return None, w
        named = boost if isinstance(boost, dict) else {None: boost}
        if not named:
            raise ValueError('boost: the dict of phrase sets is empty')
        if len(named) > qsb.MAX_SETS:
            raise ValueError(f'boost: {len(named)} phrase sets, at most MAX_SETS = {qsb.MAX_SETS} per session')
        sets = {}
        for name, ph in named.items():
            if name is False or (name is not None and not isinstance(name, str)):
                raise ValueError(f'boost: the name of a phrase set must be a string, got {name!r}')
            try:
                sets[name] = qboost.as_phrase_set(ph, self.decoder.vocabulary, w)
            except ValueError as e:
                raise ValueError(str(e) if name is None else f'{e} (set {name!r})') from None
        return sets, w

    @staticmethod
    def _beam_args(beam_width, n_best, cutoff_top_n):
        from qasr import beam as qbeam
        beam_width, n_best, cutoff_top_n = int(beam_width), int(n_best), int(cutoff_top_n)
        if not 1 <= beam_width <= qbeam.MAX_W:
            raise ValueError(f'decode: beam_width must be 1 .. {qbeam.MAX_W}, got {beam_width}')
        if not 1 <= cutoff_top_n <= qbeam.MAX_N:
            raise ValueError(f'decode: cutoff_top_n must be 1 .. {qbeam.MAX_N}, got {cutoff_top_n}')
        if not 1 <= n_best <= beam_width:
            raise ValueError(f'decode: n_best must be 1 .. beam_width, got {n_best}')
        return beam_width, n_best, cutoff_top_n

    def _lm_args(self, lm, alpha, beta):
        """the NgramLM of decode(lm=): a path is loaded once per module; the weights are refused here, before any launch"""
        if lm is None:
            return None
        from qasr import ngram
        try:
            ngram.fixed_weights(alpha, beta)
        except ValueError as e:
            raise ValueError(f'decode: {e}') from None
        if not isinstance(lm, ngram.NgramLM):
            key = os.fspath(lm)
            cache = self.__dict__.setdefault('_lm_cache', {})
            if key not in cache:
                cache[key] = ngram.NgramLM.from_arpa(key, self.decoder.vocabulary)
            lm = cache[key]
        if lm.n_labels != len(self.decoder.vocabulary):
            raise ValueError(f'decode: the language model was loaded for {lm.n_labels} labels, the decoder has '
                             f'{len(self.decoder.vocabulary)}')
        return lm

    def _mbr_args(self, who, mbr, mbr_scale, beam_width, n_best):
        """decode(mbr=)'s arguments, refused by name before anything runs: None without mbr, else (mode, scale)"""
        if mbr is None:
            return None
        from qasr import mbr as qmbr
        if mbr not in ('word', 'char'):
            raise ValueError(f"{who}: mbr must be None, 'word' or 'char', got {mbr!r}")
        if beam_width is None:
            raise ValueError(f'{who}: mbr needs beam_width (the greedy collapse has one hypothesis, nothing to re-rank)')
        if int(n_best) < 2:
            raise ValueError(f'{who}: mbr needs n_best >= 2 (a list of one row has nothing to re-rank), got {n_best}')
        try:
            qmbr.check_scale(mbr_scale, who)
        except ValueError as e:
            raise ValueError(str(e)) from None
        if mbr == 'word':
            from qasr import edit as qedit
            qedit.space_mask(list(self.decoder.vocabulary), who)
        return mbr, float(mbr_scale)

    def _mbr_rows(self, res, mbr):
        """qasr_ctc_mbr (the twin for host arrays) behind a BeamResult, over its buffers as they lie; nothing is read back"""
        from qasr import edit as qedit, mbr as qmbr
        mode, scale = mbr
        vocab = list(self.decoder.vocabulary)
        mask = qedit.space_mask(vocab, 'decode') if mode == 'word' else None
        if torch.is_tensor(res.labels) and res.labels.is_cuda:
            sp = None if mask is None else torch.from_numpy(mask).to(res.labels.device)
            return qmbr.mbr_device(res.labels, res.n_labels, res.score, res.n_hyps, len(vocab), mode=mode, is_space=sp, scale=scale)
        host = lambda t: t.numpy() if torch.is_tensor(t) else t
        return qmbr.mbr_host(host(res.labels), host(res.n_labels), host(res.score), host(res.n_hyps), len(vocab), mode=mode,
                             is_space=mask, scale=scale)

    @staticmethod
    def _mbr_order(hyps, mres):
        """the lists in MBR order, every hypothesis with posterior, mbr_risk and beam_rank; weight, wsum, risk and order are read"""
        from qasr import mbr as qmbr
        cpu = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t
        mres = qmbr.MbrResult(None, cpu(mres.weight), cpu(mres.wsum), cpu(mres.risk), cpu(mres.order), cpu(mres.ok))
        ee, post = qmbr.expected_errors(mres)
        out = []
        for b, row in enumerate(hyps):
            order = [int(k) for k in mres.order[b] if 0 <= k < len(row)]
            if len(order) != len(row):
                raise RuntimeError(f'decode: the re-ranking refused a row of utterance {b} that the beam wrote')
            for k in order:
                row[k].posterior, row[k].mbr_risk, row[k].beam_rank = float(post[b, k]), float(ee[b, k]), k
            out.append([row[k] for k in order])
        return out

    def _beam_decode(self, fwd, beam_width, n_best, cutoff_top_n, lm=None, alpha=0.0, beta=0.0, timestamps=False, boost=None,
                     posteriors=False, rows=False, mbr=None):
        """decode(beam_width=) behind any path's (log_probs, encoded lengths, tokens); the arguments passed _beam_args"""
        from qasr import beam as qbeam
        log_probs, enc_len = fwd[0], fwd[1]
        blank = len(self.decoder.vocabulary)
        if log_probs.is_cuda:
            from qasr import engine as qengine
            res = qengine.ctc_beam_search(log_probs.float(), enc_len, blank, beam_width, n_best, cutoff_top_n, lm=lm,
                                          alpha=alpha, beta=beta, boost=boost)
        else:
            res = qbeam.search_host(log_probs.float().numpy(), enc_len.numpy(), blank, beam_width, n_best, cutoff_top_n, lm,
                                    alpha, beta, boost)
        mres = None if mbr is None else self._mbr_rows(res, mbr)     # behind the beam chain, on the same stream
        if rows:                             # error_rate: the BeamResult as it lies (with mbr: its MbrResult beside it)
            if mres is not None:
                res.mbr = mres
            return res
        hyps = qbeam.to_hypotheses(res, self.decoder.vocabulary)
        if timestamps:
            self._beam_timestamps(hyps, res, log_probs, enc_len, blank, n_best, posteriors)
        if mres is not None:
            hyps = self._mbr_order(hyps, mres)
        return hyps if n_best > 1 else [h[0] for h in hyps]          # a beam over real candidates never dies: h[0] exists

    def _beam_timestamps(self, hyps, res, log_probs, enc_len, blank, n_best, posteriors=False):
        """decode(beam_width=, timestamps=True): the beam's label rows [B][n_best][T] are the targets as they lie (n_best
        problems per utterance, row pitch T; rows past n_hyps are empty targets and are dropped with their hypotheses).
        posteriors: k_post (the host modules: post_host) over the same rows behind the alignment."""
        from qasr import align as qalign
        B, nb, T = res.labels.shape
        ml = min(T, qalign.MAX_LABELS)                           # a hypothesis beyond the cap is not alignable: no times
        if log_probs.is_cuda:
            from qasr import engine as qengine
            tg = res.labels.view(B * nb, T) if ml == T else res.labels[:, :, :ml].contiguous().view(B * nb, ml)
            ares = qengine.ctc_align(log_probs.float(), enc_len, tg, res.n_labels.view(B * nb), blank, problems_per_utt=nb,
                                     want_total=False)
            post = qengine.ctc_post(log_probs.float(), enc_len, tg, res.n_labels.view(B * nb), blank, ares,
                                    problems_per_utt=nb) if posteriors else None
        else:
            ares = qalign.align_host(log_probs.float().numpy(), enc_len.numpy(), res.labels.reshape(B * nb, T)[:, :ml],
                                     res.n_labels.reshape(B * nb), blank, problems_per_utt=nb, want_total=False)
            post = qalign.post_host(log_probs.float().numpy(), enc_len.numpy(), ares.labels, ares.n_labels, blank, ares.start,
                                    ares.nframes, ares.ok, problems_per_utt=nb) if posteriors else None
        if posteriors:
            timed = qalign.post_to_hypotheses(ares, post, self.decoder.vocabulary, self.seconds_per_frame(), lens=enc_len)
        else:
            timed = qalign.to_hypotheses(ares, self.decoder.vocabulary, self.seconds_per_frame())
        for b, row in enumerate(hyps):
            for h, hyp in enumerate(row):
                t = timed[b * nb + h]
                hyp.start_s, hyp.end_s, hyp.score, hyp.words = t.start_s, t.end_s, t.score, t.words
                if posteriors:
                    hyp.post, hyp.post_min, hyp.word_post, hyp.frame_post = t.post, t.post_min, t.word_post, t.frame_post

    def _star_args(self, who, star, star_penalty):
        """The wildcard's arguments (qasr.align.STAR_RULES), refused by name before anything runs: the token (None: no
        wildcard), the wildcard's label id (len(vocabulary) + 1: one past the blank) and the penalty as float32."""
        from qasr import align as qalign
        vocab = list(self.decoder.vocabulary)
        try:
            pen = qalign.check_star_penalty(star_penalty, who)
        except ValueError as e:
            raise ValueError(str(e).replace('penalty', 'star_penalty', 1)) from None
        if star is not None:
            if not isinstance(star, str) or not star:
                raise ValueError(f'{who}: star must be a non-empty token string, got {star!r}')
            shared = sorted({ch for ch in star if any(ch in label for label in vocab)})
            if shared:
                raise ValueError(f'{who}: the star token {star!r} shares {shared!r} with the vocabulary')
        return star, len(vocab) + 1, pen

    @staticmethod
    def _star_pieces(text, token, parser, who, where):
        """A text split on the wildcard's token before the parser sees the pieces (its normaliser would drop the token): the
        pieces' label ids in order, None standing for a wildcard; a piece of nothing but spaces gives no item"""
        items = []
        for k, part in enumerate(text.split(token)):
            if k:
                items.append(None)
            if part.strip():
                ids = parser(part)
                if ids is None:
                    raise ValueError(f'{who}: {where} is rejected by the parser')
                if ids:
                    items.append([int(c) for c in ids])
        return items

    @staticmethod
    def _star_join(groups, space, wild):
        """Label ids of groups of items (a list of label ids, or None for a wildcard), in order: consecutive wildcards collapse
        to one, and when the vocabulary has a space its label stands between two neighbouring items, so a wildcard never
        touches a word.  Also, per group, (first, count) from its first to its last label that is no wildcard (None for a group
        without one)."""
        ids, spans, prev_wild = [], [], False
        for g in groups:
            first = last = None
            for it in g:
                if it is None and prev_wild:
                    continue
                if ids and space is not None:
                    ids.append(space)
                if it is None:
                    ids.append(wild)
                else:
                    real = [k for k, c in enumerate(it) if c != wild]
                    if real:
                        first = len(ids) + real[0] if first is None else first
                        last = len(ids) + real[-1] + 1
                    ids += it
                prev_wild = it is None or it[-1] == wild
            spans.append(None if first is None else (first, last - first))
        return ids, spans

    @torch.no_grad()
    def align(self, input_signal=None, input_signal_length=None, processed_signal=None, processed_signal_length=None,
              texts=None, labels=None, sample_rate=None, channels=1, star=None, star_penalty=1.0, posteriors=False):
        """Forced alignment and CTC scoring of GIVEN transcripts (an extension of the reference's API): one
        qasr.ctc.Hypothesis per utterance with the text's labels, every label's start / end time and confidence and the word
        groups of its best (Viterbi) alignment against this batch's log-probabilities, utt_score = the log-probability of that
        alignment and ctc_score = the CTC log-likelihood of the text over all alignments (qasr.align states the rules).  The
        signal arguments are forward()'s; exactly one of `texts` (strings: they pass through the CharParser the data layer
        uses - the model's vocabulary, the 'en' normaliser) and `labels` (one sequence of label ids per utterance).  A text the
        parser rejects, an id outside the vocabulary or a transcript above qasr.align.MAX_LABELS labels raises ValueError naming
        its index before anything runs.  Runs behind every path decode(beam_width=) runs behind - static engine, reserved
        engine, dynamic path (k_align on the same stream), host modules (the NumPy twin).  A transcript with more labels (plus
        adjacent repeats) than the utterance has frames is not alignable: empty time lists, scores -inf.

        star: a token string such as '*' that marks audio the transcript does not cover (qasr.align.STAR_RULES).  A text is
        split on the token before the parser sees the pieces; the pieces' labels are joined by the wildcard label, a space
        label on either side of it when the vocabulary has one, and consecutive tokens count once; in `labels` the id
        len(vocabulary) + 1 is the wildcard.  The wildcard's log-probability at a frame is the frame's best class less
        star_penalty nats (k_star in front of k_align on the same stream; 0 .. 16, default 1.0 - a starting point, not tuned
        on speech).  The hypothesis shows the token in text, carries its times and, as its score, the best value of that plane
        inside its run, lists it in words as a word of its own - where the untranscribed audio lies - and counts its emissions
        in utt_score; ctc_score is None for a transcript that holds a wildcard.  An empty token, a token that shares a
        character with the vocabulary, a star_penalty outside 0 .. 16 and the wildcard's id in labels without `star` are
        refused by name; MAX_LABELS counts wildcards.

        posteriors=True: how sure the alignment is (qasr.align.POST_RULES).  A backward pass over the same lattice (k_post
        behind k_align on the same stream; post_host on the host modules) gives the posterior of the path's own state at every
        frame - the share of the text's probability mass whose alignments sit in that state then.  The hypothesis carries post
        (per label, the mean over its run, 0 .. 1), post_min (per label, its least certain frame), word_post (one per entry of
        words: the mean over the frames of the word's labels) and frame_post (float32 log-posteriors of the frames); a transcript
        that is not alignable gets empty lists.  With a wildcard the posteriors are taken in the lattice that holds it.  Without
        posteriors=True the fields stay None and the call launches what it always did."""
        from qasr import align as qalign
        star, wild, star_pen = self._star_args('align', star, star_penalty)
        input_signal, input_signal_length = self._resample_in(input_signal, input_signal_length, sample_rate, channels)
        if (texts is None) == (labels is None):
            raise ValueError('align: give exactly one of texts and labels')
        vocab = list(self.decoder.vocabulary)
        blank = len(vocab)
        if texts is not None:
            from nemo.collections.asr.parts import parsers
            parser = parsers.make_parser(labels=vocab, name='en', unk_id=-1, blank_id=-1, do_normalize=True)
            space = vocab.index(' ') if ' ' in vocab else None
            rows = []
            for i, text in enumerate(texts):
                if star is not None and isinstance(text, str):
                    rows.append(self._star_join([self._star_pieces(text, star, parser, 'align', f'text {i}')], space, wild)[0])
                    continue
                ids = parser(text) if isinstance(text, str) else None
                if ids is None:
                    raise ValueError(f'align: text {i} is rejected by the parser')
                rows.append(ids)
        else:
            rows = [[int(c) for c in r] for r in labels]
        for i, ids in enumerate(rows):
            if star is None and wild in ids:
                raise ValueError(f'align: transcript {i} holds the wildcard label {wild}, but no star token was given')
            if any(not 0 <= c < blank and c != wild for c in ids):
                raise ValueError(f'align: transcript {i} holds a label outside the vocabulary of {blank} labels')
            if len(ids) > qalign.MAX_LABELS:
                raise ValueError(f'align: transcript {i} has {len(ids)} labels, at most {qalign.MAX_LABELS} can be aligned')
        ref = input_signal if input_signal is not None else processed_signal
        if ref is not None and len(rows) != ref.shape[0]:
            raise ValueError(f'align: {len(rows)} transcripts for a batch of {ref.shape[0]} utterances')
        fwd = self._forward(input_signal, input_signal_length, processed_signal, processed_signal_length)
        log_probs, enc_len = fwd[0], fwd[1]
        tg = np.full((len(rows), max(1, max(len(r) for r in rows))), blank, dtype=np.int32)
        for i, ids in enumerate(rows):
            tg[i, :len(ids)] = ids
        tl = np.array([len(r) for r in rows], dtype=np.int32)
        use_star = star is not None and any(wild in ids for ids in rows)      # no wildcard in any transcript: the call it was
        if log_probs.is_cuda:
            from qasr import engine as qengine
            plane = qengine.ctc_star(log_probs.float(), enc_len, star_pen) if use_star else None
            res = qengine.ctc_align(log_probs.float(), enc_len, torch.from_numpy(tg).to(log_probs.device),
                                    torch.from_numpy(tl).to(log_probs.device), blank, star=plane)
            post = qengine.ctc_post(log_probs.float(), enc_len, res.labels, res.n_labels, blank, res, star=plane) if posteriors else None
        else:
            plane = qalign.star_host(log_probs.float().numpy(), enc_len.numpy(), star_pen) if use_star else None
            res = qalign.align_host(log_probs.float().numpy(), enc_len.numpy(), tg, tl, blank, star=plane)
            post = qalign.post_host(log_probs.float().numpy(), enc_len.numpy(), tg, tl, blank, res.start, res.nframes, res.ok,
                                    star=plane) if posteriors else None
        if posteriors:
            return qalign.post_to_hypotheses(res, post, vocab, self.seconds_per_frame(), lens=enc_len, star_token=star)
        return qalign.to_hypotheses(res, vocab, self.seconds_per_frame(), star_token=star)

    def _long_transcripts(self, texts, labels, n_recordings, star=None, wild=None, star_between=False):
        """align_long's transcripts: per recording its label ids and, where an utterance list was given, the utterances as
        (text, first label, labels); utterances are joined by the space label when the vocabulary has one.  star / wild: the
        wildcard's token and label id (_star_args); star_between: a wildcard around and between the utterances of a list"""
        if (texts is None) == (labels is None):
            raise ValueError('align_long: give exactly one of texts and labels')
        vocab = list(self.decoder.vocabulary)
        blank = len(vocab)
        space = vocab.index(' ') if ' ' in vocab else None
        if star is not None:
            return self._long_transcripts_star(texts, labels, n_recordings, star, wild, star_between, vocab, space)
        given = texts if texts is not None else labels
        if len(given) != n_recordings:
            raise ValueError(f'align_long: {len(given)} transcripts for {n_recordings} recordings')
        if texts is not None:
            from nemo.collections.asr.parts import parsers
            parser = parsers.make_parser(labels=vocab, name='en', unk_id=-1, blank_id=-1, do_normalize=True)

            def ids_of(x, where):
                ids = parser(x) if isinstance(x, str) else None
                if ids is None:
                    raise ValueError(f'align_long: {where} is rejected by the parser')
                return [int(c) for c in ids], x
        else:
            def ids_of(x, where):
                ids = [int(c) for c in x]
                if wild is not None and wild in ids:
                    raise ValueError(f'align_long: {where} holds the wildcard label {wild}, but no star token was given')
                if any(not 0 <= c < blank for c in ids):
                    raise ValueError(f'align_long: {where} holds a label outside the vocabulary of {blank} labels')
                return ids, ''.join(vocab[c] for c in ids)
        rows, utts = [], []
        for r, item in enumerate(given):
            is_list = (not isinstance(item, str)) if texts is not None else (len(item) > 0 and np.ndim(item[0]) > 0)
            if not is_list:
                ids, _ = ids_of(item, f'transcript {r}')
                rows.append(ids)
                utts.append(None)
                continue
            ids, us = [], []
            for j, u in enumerate(item):
                uid, text = ids_of(u, f'utterance {j} of transcript {r}')
                if not uid:
                    raise ValueError(f'align_long: utterance {j} of transcript {r} is empty')
                if ids and space is not None:
                    ids.append(space)
                us.append((text, len(ids), len(uid)))
                ids += uid
            rows.append(ids)
            utts.append(us)
        from qasr import align as qalign
        for r, ids in enumerate(rows):
            if any(not 0 <= c < blank for c in ids):
                raise ValueError(f'align_long: transcript {r} holds a label outside the vocabulary of {blank} labels')
            if len(ids) > qalign.BAND_MAX_LABELS:
                raise ValueError(f'align_long: transcript {r} has {len(ids)} labels, at most {qalign.BAND_MAX_LABELS} can be aligned')
        return rows, utts

    def _long_transcripts_star(self, texts, labels, n_recordings, star, wild, star_between, vocab, space):
        """_long_transcripts with a wildcard token: the same rows and utterance spans, built from items (_star_pieces,
        _star_join); an utterance's span runs from its first to its last label that is no wildcard"""
        from qasr import align as qalign
        blank = len(vocab)
        given = texts if texts is not None else labels
        if len(given) != n_recordings:
            raise ValueError(f'align_long: {len(given)} transcripts for {n_recordings} recordings')
        if texts is not None:
            from nemo.collections.asr.parts import parsers
            parser = parsers.make_parser(labels=vocab, name='en', unk_id=-1, blank_id=-1, do_normalize=True)

            def items_of(x, where):
                if not isinstance(x, str):
                    raise ValueError(f'align_long: {where} is rejected by the parser')
                return self._star_pieces(x, star, parser, 'align_long', where), x
        else:
            def items_of(x, where):
                ids = [int(c) for c in x]
                if any(not 0 <= c < blank and c != wild for c in ids):
                    raise ValueError(f'align_long: {where} holds a label outside the vocabulary of {blank} labels')
                return ([ids] if ids else []), ''.join(star if c == wild else vocab[c] for c in ids)
        rows, utts = [], []
        for r, item in enumerate(given):
            is_list = (not isinstance(item, str)) if texts is not None else (len(item) > 0 and np.ndim(item[0]) > 0)
            if not is_list:
                ids, _ = self._star_join([items_of(item, f'transcript {r}')[0]], space, wild)
                rows.append(ids)
                utts.append(None)
                continue
            groups, shown = [[None]] if star_between else [], []
            for j, u in enumerate(item):
                its, text = items_of(u, f'utterance {j} of transcript {r}')
                groups.append(its)
                shown.append(text)
                if star_between:
                    groups.append([None])
            ids, spans = self._star_join(groups, space, wild)
            spans = spans[1::2] if star_between else spans
            for j, sp in enumerate(spans):
                if sp is None:
                    raise ValueError(f'align_long: utterance {j} of transcript {r} is empty')
            rows.append(ids)
            utts.append([(text, a, k) for text, (a, k) in zip(shown, spans)])
        for r, ids in enumerate(rows):
            if len(ids) > qalign.BAND_MAX_LABELS:
                raise ValueError(f'align_long: transcript {r} has {len(ids)} labels, at most {qalign.BAND_MAX_LABELS} can be aligned')
        return rows, utts

    @torch.no_grad()
    def align_long(self, input_signal, input_signal_length, texts=None, labels=None, window_s=30.0, overlap_s=4.0, guard_s=1.0,
                   batch_size=32, seam='blank', band_states=None, sample_rate=None, channels=1, star=None, star_penalty=1.0,
                   star_between=False, posteriors=False):
        """CTC segmentation of long recordings (an extension; the job of the reference's tools/ctc_segmentation, on the
        device): input_signal [R, S] with input_signal_length samples each and, per recording, its whole transcript ->
        List[qasr.ctc.Hypothesis], one per recording, with every label's and word's times in seconds of the recording,
        utt_score = the log-probability of the alignment, ctc_score = None (unless posteriors=True, below) and seams_s as
        decode_long's.  Exactly one of `texts` and `labels`; texts[r] is a string, or a list of utterance strings (labels[r]:
        a sequence of ids, or a list of such): utterances are joined by the space label when the vocabulary has one, by
        nothing otherwise, an empty utterance is refused by name, and the hypothesis then carries `segments`, one
        qasr.ctc.Segment(text, start_s, end_s, score) per utterance - from the first frame of its first label to the end of its
        last label's run, score = the min-mean confidence of qasr.align.segment_scores over those frames.

        The windows run as in decode_long (k_cut, batches of batch_size through the reserved engine, which writes
        log-probabilities here), the log-probability rows go through k_stitch as one more plane, and one launch of
        k_align_band aligns every recording against its transcript inside a band of band_states lattice states (256, 1024
        or 4352; None: the smallest that holds the longest transcript whole, else 4352) that follows the alignment
        (qasr.align.BAND_RULES).  A transcript whose path the band loses - or that has more labels than the recording has
        frames - keeps its text; its times are empty and its scores -inf.  CPU inputs run the NumPy twins.  The stitched
        log-probabilities take 4 * classes bytes per frame of every recording, and the windows as much again.

        star, star_penalty: the wildcard of align() - the token inside a text or an utterance, the id len(vocabulary) + 1 in
        labels - with k_star in front of k_align_band.  star_between=True puts a wildcard before the first utterance of an
        utterance list, between every two and behind the last (space labels around each when the vocabulary has a space; the
        token is star, '*' when star is None), for recordings whose transcript skips what lies between the utterances.
        `segments` stay one per utterance, from its first to its last label that is no wildcard: the frames of the wildcards
        in between belong to no segment.  The hypothesis shows the tokens in text and in words.

        posteriors=True: how sure the alignment is (qasr.align.POST_BAND_RULES).  The banded alignment also returns the band's
        trajectory, and k_post_band (CPU inputs: post_band_host) follows on the same stream with a forward and a backward pass
        inside that band.  Every hypothesis gains post, post_min, word_post and frame_post with the meaning
        align(posteriors=True) gives them, every Segment gains post - the mean of exp(frame_post) over its frames - and ctc_score
        is filled: total / 2^16, the log-likelihood of the alignments that stay inside the band, a lower bound on the full
        lattice's (None when the transcript holds a wildcard, as in align).  A lost path keeps empty lists and Segment.post None.
        Without posteriors=True the call launches, allocates and returns what it always did."""
        from qasr import align as qalign, engine as qengine
        if input_signal is None or input_signal_length is None:
            raise ValueError('align_long: input_signal and input_signal_length are required')
        if seam not in ('blank', 'middle'):
            raise ValueError(f"align_long: seam must be 'blank' or 'middle', got {seam!r}")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f'align_long: batch_size must be at least 1, got {batch_size}')
        if band_states is not None:
            try:
                band_states = qalign.pick_band_states(0, band_states)
            except ValueError as e:
                raise ValueError(f'align_long: {e}') from None
        star, wild, star_pen = self._star_args('align_long', '*' if star is None and star_between else star, star_penalty)
        signal, length = self._resample_in(input_signal, input_signal_length, sample_rate, channels)
        if signal.dim() != 2:
            raise ValueError(f'align_long: input_signal must be [R, S], got {tuple(signal.shape)}')
        rows, utts = self._long_transcripts(texts, labels, signal.shape[0], star, wild, star_between)
        signal = signal.float()
        lens_host = length.detach().cpu().long().clamp(max=signal.shape[1])
        plan = self._long_plan(lens_host.numpy(), window_s, overlap_s, guard_s)      # refuses its arguments by name
        vocab = list(self.decoder.vocabulary)
        blank = len(vocab)
        if plan.Wn == plan.R:                # no recording is longer than a window: nothing is cut
            windows, wlens = signal, lens_host.to(signal.device)
        else:
            windows, wlens = qengine.longform_cut(signal, lens_host.to(signal.device), plan)
        toks, fs, enc, planes = self._long_windows(plan, windows, wlens, length.dtype, batch_size, 'logp')
        out, total, seams = qengine.longform_stitch(plan, enc, toks, fs, planes, blank, seam)
        logp = out[2]
        tg = np.full((len(rows), max(1, max(len(r) for r in rows))), blank, dtype=np.int32)
        for i, ids in enumerate(rows):
            tg[i, :len(ids)] = ids
        tl = np.array([len(r) for r in rows], dtype=np.int32)
        bw = qalign.pick_band_states(tg.shape[1], band_states)
        use_star = star is not None and any(wild in ids for ids in rows)      # no wildcard in any transcript: the call it was
        if logp.is_cuda:
            plane = qengine.ctc_star(logp, total, star_pen) if use_star else None
            res = qengine.ctc_align_band(logp, total, torch.from_numpy(tg).to(logp.device), torch.from_numpy(tl).to(logp.device),
                                         blank, band_states=bw, want_band_base=bool(posteriors), star=plane)
            post = qengine.ctc_post_band(logp, total, res.labels, res.n_labels, blank, res, star=plane) if posteriors else None
        else:
            plane = qalign.star_host(logp.numpy(), total.numpy(), star_pen) if use_star else None
            res = qalign.align_band_host(logp.numpy(), total.numpy(), tg, tl, blank, band_states=bw, want_band_base=bool(posteriors),
                                         star=plane)
            post = qalign.post_band_host(logp.numpy(), total.numpy(), tg, tl, blank, res.start, res.nframes, res.ok, res.band_base, bw,
                                         star=plane) if posteriors else None
        spf_s = self.seconds_per_frame()
        if posteriors:
            res.total = post.total                                  # ctc_score: the likelihood inside the band
            hyps = qalign.post_to_hypotheses(res, post, vocab, spf_s, lens=total, star_token=star)
            post_ok, frame_post = qalign._np(post.ok), qalign._np(post.frame_post)
            for h, p_ok in zip(hyps, post_ok):
                if not p_ok and h.ctc_score is not None:
                    h.ctc_score = float('-inf')
        else:
            hyps = qalign.to_hypotheses(res, vocab, spf_s, star_token=star)
        seams_h = seams.cpu().numpy()
        if any(u is not None for u in utts):
            ok, start, nframes = (qalign._np(x) for x in (res.ok, res.start, res.nframes))
            frame_logp = qalign._np(res.frame_logp)
        for r, h in enumerate(hyps):
            w0, n = int(plan.first[r]), int(plan.count[r])
            h.seams_s = [float(seams_h[w]) * spf_s for w in range(w0 + 1, w0 + n)] if n > 1 else None
            if utts[r] is None:
                continue
            from qasr.ctc import Segment
            if not ok[r]:
                h.segments = [Segment(text, None, None, float('-inf')) for text, _, _ in utts[r]]
                continue
            f0 = np.array([start[r, a] for _, a, _ in utts[r]], dtype=np.int64)
            f1 = np.array([start[r, a + k - 1] + nframes[r, a + k - 1] for _, a, k in utts[r]], dtype=np.int64)
            sc = qalign.segment_scores(frame_logp[r], f0, f1)
            h.segments = [Segment(text, float(a) * spf_s, float(b) * spf_s, float(c)) for (text, _, _), a, b, c in zip(utts[r], f0, f1, sc)]
            if posteriors and post_ok[r]:
                pr = np.exp(frame_post[r].astype(np.float64) / qalign.ONE)
                for seg, a, b in zip(h.segments, f0, f1):
                    seg.post = float(pr[a:b].mean())
        return hyps

    def _spot_args(self, who, keywords, labels, threshold, max_span_s, max_hits):
        """The keyword list of spot / spot_long, refused by name before anything runs: (the keywords as given, targets int32
        [K, ML], target_lens int32 [K], threshold, max_span in frames, max_hits)"""
        from qasr import spot as qspot
        if (keywords is None) == (labels is None):
            raise ValueError(f'{who}: give exactly one of keywords and labels')
        vocab = list(self.decoder.vocabulary)
        blank = len(vocab)
        given = list(keywords if keywords is not None else labels)
        if not given:
            raise ValueError(f'{who}: the keyword list is empty')
        if keywords is not None:
            from nemo.collections.asr.parts import parsers
            parser = parsers.make_parser(labels=vocab, name='en', unk_id=-1, blank_id=-1, do_normalize=True)
            rows = []
            for i, text in enumerate(given):
                ids = parser(text) if isinstance(text, str) else None
                if ids is None:
                    raise ValueError(f'{who}: keyword {i} is rejected by the parser')
                rows.append([int(c) for c in ids])
        else:
            rows = [[int(c) for c in r] for r in given]
            given = [tuple(r) for r in rows]
        for i, ids in enumerate(rows):
            if not ids:
                raise ValueError(f'{who}: keyword {i} is empty')
            if len(ids) > qspot.MAX_LABELS:
                raise ValueError(f'{who}: keyword {i} has {len(ids)} labels, at most {qspot.MAX_LABELS} can be spotted')
            if any(not 0 <= c < blank for c in ids):
                raise ValueError(f'{who}: keyword {i} holds a label outside the vocabulary of {blank} labels')
        qspot.check_threshold(threshold, who)
        try:
            span = int(round(float(max_span_s) / self.seconds_per_frame()))
        except (TypeError, ValueError, OverflowError):
            span = 0
        if not 1 <= span <= qspot.MAX_SPAN:
            raise ValueError(f'{who}: max_span_s {max_span_s!r} is {span} frames, outside 1 .. {qspot.MAX_SPAN}')
        if int(max_hits) < 1:
            raise ValueError(f'{who}: max_hits must be at least 1, got {max_hits!r}')
        tg = np.full((len(rows), max(len(r) for r in rows)), blank, dtype=np.int32)
        for i, ids in enumerate(rows):
            tg[i, :len(ids)] = ids
        return given, tg, np.array([len(r) for r in rows], dtype=np.int32), float(threshold), span, int(max_hits)

    def _spot_rows(self, log_probs, lens, tg, tl, threshold, span, max_hits):
        """k_star (penalty 0) and k_spot on the current stream for cuda rows, the NumPy twins otherwise: a qasr.spot.SpotResult"""
        from qasr import align as qalign, spot as qspot
        blank = len(self.decoder.vocabulary)
        if log_probs.is_cuda:
            from qasr import engine as qengine
            lp = log_probs.float()
            plane = qengine.ctc_star(lp, lens, 0.0)
            return qengine.ctc_spot(lp, lens, plane, torch.from_numpy(tg).to(lp.device), torch.from_numpy(tl).to(lp.device), blank,
                                    threshold, span, max_hits)
        lp, ln = log_probs.float().numpy(), lens.numpy()
        return qspot.spot_host(lp, ln, qalign.star_host(lp, ln, 0.0), tg, tl, blank, qspot.check_threshold(threshold, 'spot'), span,
                               max_hits)

    @torch.no_grad()
    def spot(self, input_signal=None, input_signal_length=None, processed_signal=None, processed_signal_length=None,
             keywords=None, labels=None, threshold=-1.0, max_span_s=10.0, max_hits=16, sample_rate=None, channels=1):
        """Keyword spotting (an extension of the reference's API): where each of a list of phrases occurs in every utterance of
        the batch, and how well it matches, without going through the 1-best transcript - List[List[qasr.ctc.KeywordHit]], one
        list per utterance, sorted by start.  The signal arguments are forward()'s; exactly one of `keywords` (strings: they
        pass through the CharParser the data layer uses, as align()'s texts do) and `labels` (one sequence of label ids per
        keyword).  Every keyword's CTC lattice runs over the frames with a free start and a free end, scored by the likelihood
        ratio against the frame's best class (qasr.spot.SPOT_RULES): a hit's score is the mean of that ratio over its span in
        nats per frame, <= 0, and 0 means the keyword IS the greedy path there.  threshold: the lowest mean a hit may have,
        -16 .. 0 nats per frame; max_span_s: the longest hit; max_hits: hits kept per keyword and utterance, the earliest first.
        threshold = -1.0 and max_span_s = 10 are starting points, not tuned on speech.  Runs behind every path align() runs
        behind - static engine, reserved engine, dynamic path (k_star with penalty 0, then k_spot, on the same stream), host
        modules (the NumPy twins).  An empty list, an empty keyword, a keyword of more than 127 labels or that the parser
        rejects, an id outside the vocabulary, a threshold outside -16 .. 0 and a max_span_s that rounds to fewer than 1 or more
        than 65536 frames are refused by name before anything runs."""
        from qasr import spot as qspot
        given, tg, tl, threshold, span, max_hits = self._spot_args('spot', keywords, labels, threshold, max_span_s, max_hits)
        input_signal, input_signal_length = self._resample_in(input_signal, input_signal_length, sample_rate, channels)
        fwd = self._forward(input_signal, input_signal_length, processed_signal, processed_signal_length)
        res = self._spot_rows(fwd[0], fwd[1], tg, tl, threshold, span, max_hits)
        return qspot.to_hits(res, given, self.seconds_per_frame())

    @torch.no_grad()
    def spot_long(self, input_signal, input_signal_length, keywords=None, labels=None, window_s=30.0, overlap_s=4.0, guard_s=1.0,
                  batch_size=32, seam='blank', threshold=-1.0, max_span_s=10.0, max_hits=16, sample_rate=None, channels=1):
        """spot() for long recordings: input_signal [R, S] with input_signal_length samples each -> one list of
        qasr.ctc.KeywordHit per recording, times in seconds of the recording.  The windows run as in align_long (k_cut, batches
        of batch_size through the reserved engine with log-probabilities, k_stitch with the log-probability rows as a plane);
        then one k_star launch and one k_spot launch cover the stitched rows of every recording, so a keyword that straddles a
        seam is scored over the stitched frames like any other.  CPU inputs run the NumPy twins.  The keyword arguments and
        their refusals are spot()'s, the window arguments and theirs align_long's."""
        from qasr import engine as qengine, spot as qspot
        if input_signal is None or input_signal_length is None:
            raise ValueError('spot_long: input_signal and input_signal_length are required')
        if seam not in ('blank', 'middle'):
            raise ValueError(f"spot_long: seam must be 'blank' or 'middle', got {seam!r}")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f'spot_long: batch_size must be at least 1, got {batch_size}')
        given, tg, tl, threshold, span, max_hits = self._spot_args('spot_long', keywords, labels, threshold, max_span_s, max_hits)
        signal, length = self._resample_in(input_signal, input_signal_length, sample_rate, channels)
        if signal.dim() != 2:
            raise ValueError(f'spot_long: input_signal must be [R, S], got {tuple(signal.shape)}')
        signal = signal.float()
        lens_host = length.detach().cpu().long().clamp(max=signal.shape[1])
        plan = self._long_plan(lens_host.numpy(), window_s, overlap_s, guard_s)      # refuses its arguments by name
        blank = len(self.decoder.vocabulary)
        if plan.Wn == plan.R:                # no recording is longer than a window: nothing is cut
            windows, wlens = signal, lens_host.to(signal.device)
        else:
            windows, wlens = qengine.longform_cut(signal, lens_host.to(signal.device), plan)
        toks, fs, enc, planes = self._long_windows(plan, windows, wlens, length.dtype, batch_size, 'logp')
        out, total, _ = qengine.longform_stitch(plan, enc, toks, fs, planes, blank, seam)
        res = self._spot_rows(out[2], total, tg, tl, threshold, span, max_hits)
        return qspot.to_hits(res, given, self.seconds_per_frame())

    @staticmethod
    def _frame_scores(log_probs, tokens):
        return log_probs.float().gather(2, tokens.long().unsqueeze(-1)).squeeze(-1)

    def _collapse(self, log_probs, tokens, enc_len):
        """decode() behind a path that returned log-probabilities: frame scores = log_probs at the tokens"""
        from qasr import ctc as qctc
        blank = len(self.decoder.vocabulary)
        fs = self._frame_scores(log_probs, tokens)
        if tokens.is_cuda:
            from qasr import engine as qengine
            return qengine.ctc_collapse(tokens.to(torch.int32), fs, enc_len.to(torch.int32), blank=blank)
        return qctc.collapse_host(tokens.numpy(), fs.numpy(), enc_len.numpy(), blank=blank)

    def _forward(self, input_signal=None, input_signal_length=None, processed_signal=None,
                 processed_signal_length=None, decode=False):
        """forward(); decode=True returns the CTC collapse of the batch (a qasr.ctc.CtcResult) instead of the triple;
        decode='frames' (decode_long) returns (tokens, frame scores, encoded lengths) - on the static and the reserved
        engine from the decoder kernel itself, without log-probabilities"""
        has_in = input_signal is not None and input_signal_length is not None
        has_pr = processed_signal is not None and processed_signal_length is not None
        if has_in == has_pr:
            raise ValueError(f"{self} Arguments ``input_signal`` and ``input_signal_length`` are mutually exclusive "
                             " with ``processed_signal`` and ``processed_signal_len`` arguments.")
        ref = input_signal if has_in else processed_signal
        if self.engine_ready():
            if not ref.is_cuda:
                raise RuntimeError('the calibrated integer model runs on the MI355X HIP engine only: move the inputs '
                                   'to cuda (there is no CPU fallback for the quantised inference path)')
            if self._reserve is not None:                        # reserve(): ragged batches on the reserved engine
                out = self._ragged_forward(has_in, input_signal, input_signal_length, processed_signal,
                                           processed_signal_length, decode)
                if out is not None:
                    return out
                if not self._ragged_warned:
                    import warnings
                    warnings.warn(f'a batch of shape {tuple(ref.shape)} lies outside the reserved envelope (max_batch, '
                                  f'max_seconds) = {self._reserve}: such batches run on the unreserved engine')
                    self._ragged_warned = True
            eng = self._get_engine(ref.device)
            f = self.preprocessor.featurizer
            if has_in and self._frontend_hip_supported() and f.pad_to > 0:
                # audio -> tokens as one engine call (qasr_engine_forward_audio): front-end, encoder and decoder replay as
                # one hipGraph launch when the caller keeps its buffers
                sig = input_signal.float().contiguous()
                if f.dither > 0:
                    sig = sig + f.dither * torch.randn_like(sig)
                fb, plan = self._frontend_plan_for(ref.device)
                audio_lens = input_signal_length.to(device=ref.device, dtype=torch.int32).contiguous()
                window = f.window.to(device=ref.device, dtype=torch.float32).contiguous()
                if decode:                                       # tokens only: the scores come from the decoder kernel
                    out = eng.forward_audio(sig, audio_lens, fb, window, plan, float(f.preemph), int(f.pad_to),
                                            want_logp=False, decode=True)
                    return (out[1], out[3].frame_score, out[2]) if decode == 'frames' else out[3]
                log_probs, tokens, enc_len = eng.forward_audio(sig, audio_lens, fb, window, plan, float(f.preemph), int(f.pad_to))
                return log_probs, enc_len.long(), tokens.long()
            if has_in:
                processed_signal, processed_signal_length = self._frontend_hip(input_signal, input_signal_length)
            if decode:
                out = eng.forward(processed_signal.float(), processed_signal_length, want_logp=False, decode=True)
                return (out[1], out[3].frame_score, out[2]) if decode == 'frames' else out[3]
            log_probs, tokens, enc_len = eng.forward(processed_signal.float(), processed_signal_length)
            return log_probs, enc_len.long(), tokens.long()
        if ref.is_cuda and self.dynamic_ready():
            runner = self._get_dynamic_runner(ref.device)
            if runner is not None:                               # dynamic-quantisation device path
                if has_in:
                    processed_signal, processed_signal_length = self._frontend_hip(input_signal, input_signal_length)
                out = runner.forward(processed_signal.float(), processed_signal_length)
                if decode == 'frames':
                    return out['tokens'], self._frame_scores(out['log_probs'], out['tokens']), out['enc_len']
                if decode:
                    return self._collapse(out['log_probs'], out['tokens'], out['enc_len'])
                return out['log_probs'], out['enc_len'].long(), out['tokens'].long()
        if has_in:
            processed_signal, processed_signal_length = self.preprocessor(input_signal=input_signal,
                                                                          length=input_signal_length)
        encoded, encoded_len, encoded_sf = self.encoder(audio_signal=processed_signal, length=processed_signal_length)
        log_probs = self.decoder(encoder_output=encoded, encoder_output_scaling_factor=encoded_sf)
        if decode == 'frames':
            tokens = log_probs.argmax(dim=-1, keepdim=False)
            return tokens, self._frame_scores(log_probs, tokens), encoded_len
        if decode:
            return self._collapse(log_probs, log_probs.argmax(dim=-1, keepdim=False), encoded_len)
        return log_probs, encoded_len, log_probs.argmax(dim=-1, keepdim=False)


class StreamSession:
    """EncDecCTCModel.stream(): the live streams of one model.  The host keeps counts it already has (samples per stream, the
    deltas read back so far); everything a step computes from lives on the device."""

    def __init__(self, model, max_streams, plan, tail, rs_plan=None, beam=None, bplan=None, endpoint=None, eplan=None, spot=None):
        self.model, self.S, self.plan, self.tail = model, max_streams, plan, tail
        # keyword spotting across steps (STREAM_SPOT_RULES): the StreamSpot, the keywords as given and the StreamSpotPlan
        self.spot, self._sp_given, self.splan = spot if spot is not None else (None, None, None)
        self._hits = []                      # final StreamHits that take_hits() has not handed out yet
        self._pending = {}                   # slot -> the KeywordHits that were open after the slot's last step
        self.decoded_hits = []               # decode_stream(spot=): the last call's StreamHits per recording
        self.endpoint, self.eplan = endpoint, eplan      # qasr.stream_ep.Endpointing / EndpointPlan: utterance boundaries
        self._utts = []                      # finished StreamUtterances that take_utterances() has not handed out yet
        self.beam, self.bplan = beam, bplan  # qasr.stream_beam.StreamBeam / StreamBeamPlan: the beam search across steps
        # phrase boosting across steps (STREAM_BOOST_RULES): the compiled sets in the order of their indices, and their names
        named = beam.boost if beam is not None and beam.boost is not None else None
        self._sets = None if named is None else list(named.values())
        self._set_index = None if named is None else {name: k for k, name in enumerate(named)}
        self.rs_plan = rs_plan               # qasr.stream_rs.StreamResamplePlan: the streams carry PCM at another rate
        self.closing_updates = []            # (resampled streams) the StreamUpdates of steps the last close() completed
        self._open = {}                      # slot -> dict(received, begin, deltas)
        self._dev = None                     # decided by the first push: a cuda device, or 'cpu'
        self._state = None
        self._own = False
        self.steps = 0
        self.served = None                   # after close_all(): the class that ran the steps' forwards ('Engine', 'DynamicRunner', 'NoneType': host modules)
        if model.engine_ready():             # the calibrated model: one reservation for the session's lifetime
            self._saved = (model._reserve, getattr(model, '_reserve_logp', True))
            model.reserve(max_streams, plan.Wl / float(plan.sample_rate))
            model._reserve_logp = beam is not None or spot is not None       # the beam search and the spotter read log-probabilities
            self._own = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close_all()

    def close_all(self):
        """Ends the session: open streams are dropped (close() them first for their hypotheses) and the caller's
        reservation is restored."""
        self._open.clear()
        if self.served is None:              # (kept for reports: the session's engine goes with its reservation)
            m = self.model
            self.served = type(getattr(m, '_ragged_engine', None) or getattr(m, '_engine', None)).__name__
        if self._own:
            res, logp = self._saved
            self.model.reserve(*(res if res is not None else (None, None)))
            self.model._reserve_logp = logp
            self._own = False

    def open(self, slot=None, boost=None):
        """A free slot (or `slot`) for a new stream.  boost: with StreamBeam(boost=<one set>) every stream uses the set and
        boost=False opts this one out; with a dict of sets boost='name' picks one and None means no boosting."""
        bset = -1
        if self._sets is None:
            if boost is not None and boost is not False:
                raise ValueError(f'stream: open(boost={boost!r}): the session has no phrase set (give StreamBeam(boost=...))')
        elif boost is False:
            pass
        elif None in self._set_index:        # a single set
            if boost is not None:
                raise ValueError(f'stream: open(boost={boost!r}): the session has one unnamed phrase set; pass nothing, or False')
            bset = 0
        elif boost is not None:
            if boost not in self._set_index:
                raise ValueError(f'stream: open(boost={boost!r}): no such phrase set (sets: {sorted(self._set_index)})')
            bset = self._set_index[boost]
        if slot is None:
            free = [s for s in range(self.S) if s not in self._open]
            if not free:
                raise ValueError(f'stream: all max_streams = {self.S} streams are open')
            slot = free[0]
        slot = int(slot)
        if not 0 <= slot < self.S or slot in self._open:
            raise ValueError(f'stream: slot {slot} is already open or outside 0 .. max_streams - 1 = {self.S - 1}')
        self._open[slot] = dict(received=0, begin=True, deltas=[], in_received=0, fmt=None, beam_begin=True, ep_begin=True,
                                label_base=0, boost_set=bset, spot_begin=True)
        self._pending.pop(slot, None)
        return slot

    # ---- the three steps, on the device or as the twins
    def _setup(self, device):
        from qasr import engine as qengine, stream as qstream, stream_rs as qsrs
        if self._dev is not None:
            if self._dev != device:
                raise ValueError(f'stream: the session runs on {self._dev}, got a tensor on {device}')
            return
        self._dev = device
        if self.rs_plan is not None:
            if device.type == 'cuda':
                self._rs_state = qengine.stream_rs_state(self.S, self.rs_plan, device)
                self._rs_work = qengine.stream_rs_work(self.S, device)
                self._rs_out = tuple(torch.empty(self.S, device=device, dtype=torch.int32) for _ in range(3))
                qengine.resample_plan(self.rs_plan.resample_plan, device)        # the table's upload, outside any capture
            else:
                self._rs_state = qsrs.ResampleState(self.S, self.rs_plan)
        if device.type == 'cuda':
            self._state = qengine.stream_state(self.S, self.plan, device)
            self._win = (torch.empty(self.S, self.plan.Wl, device=device), torch.empty(self.S, device=device, dtype=torch.int32),
                         torch.empty(self.S, device=device, dtype=torch.int32))
            self._out = qengine.stream_emit_buffers(self.S, self.plan, device, tail=self.tail)
            if self.endpoint is not None:
                self._ep_state = qengine.stream_ep_state(self.S, device)
                self._ep_out = qengine.stream_endpoint_buffers(self.S, self.eplan, device)
            if self.spot is not None:        # the keywords: uploaded once, held here
                self._sp_state = qengine.stream_spot_state(self.S, self.splan, device)
                self._sp_out = qengine.stream_spot_buffers(self.S, self.splan, device)
                self._sp_kw = qengine.stream_spot_keywords(self.splan, device)
                self._sp_plane = None
            if self.beam is not None:
                if self._sets is None:
                    self._bstate = qengine.stream_beam_state(self.S, self.bplan, device)
                    self._bout = qengine.stream_beam_buffers(self.S, self.bplan, device, self.beam.lm is not None)
                else:                        # the sets: packed, checked (qasr_boost_check) and uploaded once, held here
                    self._bstate = qengine.stream_beam_boost_state(self.S, self.bplan, device)
                    self._bout = qengine.stream_beam_boost_buffers(self.S, self.bplan, device, self.beam.lm is not None)
                    self._set_blobs = [qengine.boost_device(bs, device) for bs in self._sets]
                if self.endpoint is not None:                                    # cuts: k_stream_beam_ep's outputs instead
                    self._bout = qengine.stream_beam_ep_buffers(self.S, self.bplan, self.eplan.max_records, device, self.beam.lm is not None)
                self._cand = None
                qengine.lae_table_device(device)                                 # the uploads, outside any capture
                if self.beam.lm is not None:
                    qengine.lm_device(self.beam.lm, device)
        else:
            self._state = qstream.StreamState(self.S, self.plan)
            if self.endpoint is not None:
                from qasr import stream_ep as qse
                self._ep_state = qse.EpState(self.S)
            if self.spot is not None:
                from qasr import stream_spot as qss
                self._sp_state = qss.SpotState(self.S, self.splan)
            if self.beam is not None:
                from qasr import stream_beam as qsb
                self._bstate = qsb.StreamBeamState(self.S, self.bplan, check=False)

    def _i32(self, x):
        return torch.tensor(x, dtype=torch.int32).to(self._dev)

    def _push(self, slots, flags, n_new, chunk):
        from qasr import engine as qengine, stream as qstream
        if self._dev.type == 'cuda':
            qengine.stream_push(self._state, self.S, self.plan, self._i32(slots), self._i32(flags), self._i32(n_new), chunk)
        else:
            qstream.push_host(self._state, slots, flags, n_new, chunk.numpy())

    def _push_rs(self, slots, flags, n_in, out_limit, chunk):
        """one qasr_stream_rs_push (or its twin): append, then produce; nothing is read back"""
        from qasr import engine as qengine, stream_rs as qsrs
        if self._dev.type == 'cuda':
            B = len(slots)
            qengine.stream_rs_push(self._state, self._rs_state, self.S, self.rs_plan, self._i32(slots), self._i32(flags), self._i32(n_in),
                                   self._i32(out_limit), chunk, work=self._rs_work, out=tuple(t[:B] for t in self._rs_out))
        else:
            qsrs.push_rs_host(self._state, self._rs_state, slots, flags, n_in, out_limit, chunk.numpy())

    def _updates(self, stepping):
        """a step for the slots that filled a chunk; its deltas are kept and returned as StreamUpdates"""
        from qasr import ctc as qctc
        vocab, spf_s, ups = self.model.decoder.vocabulary, self.plan.seconds_per_frame(), []
        if self.beam is not None:
            step = self._step_beam_ep if self.endpoint is not None else self._step_beam
            for s, row in zip(stepping, step(stepping, False)):
                lab, fr = row['labels'], row['frames']
                if self.endpoint is None:
                    self._open[s]['deltas'].append((lab, fr))
                ups.append(qctc.StreamUpdate(s, lab.tolist(), ''.join(vocab[i] for i in lab.tolist()),
                                             (fr.astype(np.float64) * spf_s).tolist(), ((fr + 1).astype(np.float64) * spf_s).tolist(),
                                             [], ''.join(vocab[i] for i in row['tail']) if self.tail else ''))
            return ups
        for s, (lab, start, nfr, sc, _, tl) in zip(stepping, self._step(stepping, False)):
            self._open[s]['deltas'].append((lab, start, nfr, sc))
            self._cut(s)
            ups.append(qctc.StreamUpdate(s, lab.tolist(), ''.join(vocab[i] for i in lab.tolist()),
                                         (start.astype(np.float64) * spf_s).tolist(),
                                         ((start + nfr).astype(np.float64) * spf_s).tolist(),
                                         sc.astype(np.float64).tolist(), ''.join(vocab[i] for i in tl)))
        return ups

    def _rounds_rs(self, slots, n_in, chunk, flush=False):
        """The protocol of a resampled session for one piece (at most Ain frames per row): append and produce up to the
        chunk's end, step the rows that filled a chunk, and produce and step again until no ready output is left.  The
        host mirrors in_received and received with the plan's integer formulas."""
        from qasr import stream as qstream, stream_rs as qsrs
        rp, C, ch, updates = self.rs_plan, self.plan.C, self.rs_plan.channels, []
        while slots:
            flags, limit, stepping, more = [], [], [], []
            for s, n in zip(slots, n_in):
                st = self._open[s]
                flags.append((qstream.BEGIN if st['begin'] else 0) | (qsrs.FLUSH if flush else 0))
                limit.append(C - st['received'] % C)
                st['begin'] = False
                st['in_received'] += n
                target = rp.out_len(st['in_received']) if flush else rp.ready(st['in_received'])
                k = max(0, min(target - st['received'], limit[-1], C))
                st['received'] += k
                if k and st['received'] % C == 0:
                    stepping.append(s)
                if target > st['received']:
                    more.append(s)
            self._push_rs(slots, flags, n_in, limit, chunk)
            if stepping:
                updates += self._updates(stepping)
            slots, n_in = more, [0] * len(more)
            chunk = chunk[:len(more), :ch] if len(more) else chunk             # produce only: the rows' frames are not read
        return updates

    def _push_resampled(self, slots, signal, lengths):
        rp, ch = self.rs_plan, self.rs_plan.channels
        if signal.shape[1] % ch:
            raise ValueError(f'stream: a signal row of {signal.shape[1]} samples is no multiple of {ch} channels')
        S = signal.shape[1] // ch
        lens = [S] * len(slots) if lengths is None else [int(x) for x in torch.as_tensor(lengths).tolist()]
        if len(lens) != len(slots) or any(not 0 <= n <= S for n in lens):
            raise ValueError(f'stream: lengths {lens} must be one per slot, each within 0 .. {S} frames')
        for s in slots:
            fmt = self._open[s]['fmt']
            if fmt is not None and fmt != signal.dtype:
                raise ValueError(f'stream: slot {s} carries the sample format {fmt} since its first push, got {signal.dtype}')
        self._setup(signal.device)
        for s in slots:
            self._open[s]['fmt'] = signal.dtype
        updates, off = [], 0
        while off < max(lens + [0]):
            rows = [i for i in range(len(slots)) if off < lens[i]]
            n_in = [min(rp.Ain, lens[i] - off) for i in rows]
            w = max(n_in)
            if len(rows) == len(slots):
                chunk = signal[:, off * ch:(off + w) * ch]
            else:
                chunk = signal[rows, off * ch:(off + w) * ch]
            updates += self._rounds_rs([slots[i] for i in rows], n_in, chunk.contiguous())
            off += rp.Ain
        return updates

    def take_utterances(self):
        """(endpoint=) the utterances that ended since the last call, in the order they ended; the queue is cleared"""
        if self.endpoint is None:
            raise ValueError('stream: take_utterances needs a session opened with endpoint=')
        out, self._utts = self._utts, []
        return out

    def _cut(self, slot, records=None):
        """(endpoint=) the records the last step wrote for `slot`: each takes its labels off the front of the slot's deltas
        and becomes a queued StreamUtterance.  Returns the last one's Hypothesis (None: no record)."""
        if self.endpoint is None:
            return None
        from qasr import ctc as qctc, stream_ep as qse
        st, hyp = self._open[slot], None
        vocab, spf_s = self.model.decoder.vocabulary, self.plan.seconds_per_frame()
        for r in (self._ep_rows.pop(slot) if records is None else records):
            (lab, start, nfr, sc), st['deltas'] = qse.split_labels(st['deltas'], st['label_base'], r[qse.R_LABEL_END])
            st['label_base'] = int(r[qse.R_LABEL_END])
            res = qctc.CtcResult(lab[None], np.array([len(lab)], dtype=np.int32), start[None], nfr[None], sc[None],
                                 qse.record_score(r).reshape(1), len(vocab))
            hyp = qctc.to_hypotheses(res, vocab, spf_s)[0]
            sp = int(r[qse.R_SP_FIRST]) >= 0
            self._utts.append(qctc.StreamUtterance(slot, int(r[qse.R_INDEX]), qse.REASONS[int(r[qse.R_REASON])],
                                                   int(r[qse.R_FIRST]) * spf_s, int(r[qse.R_END]) * spf_s,
                                                   int(r[qse.R_SP_FIRST]) * spf_s if sp else None,
                                                   (int(r[qse.R_SP_LAST]) + 1) * spf_s if sp else None, hyp))
        return hyp

    def _endpoint(self, slots, end, sl, tok, fs, enc, first, emit, blank):
        """(endpoint=) the endpoint launch (or its twin) behind a step's emit; keeps the rows' records for _cut"""
        from qasr import engine as qengine, stream as qstream, stream_ep as qse
        B = len(slots)
        flags = [(qstream.END if end else 0) | (qstream.BEGIN if self._open[s]['ep_begin'] else 0) for s in slots]
        for s in slots:
            self._open[s]['ep_begin'] = False
        if self._dev.type == 'cuda':
            out = qse.EpStepBatch(*[getattr(self._ep_out, n)[:B] for n in ('records', 'n_records', 'status')])
            qengine.stream_endpoint(self._state, self._ep_state, self.S, self.plan, self.eplan, sl, self._i32(flags), tok, fs, enc, first,
                                    emit, blank, out=out)
            o = qse.EpStepBatch(out.records.cpu().numpy(), out.n_records.cpu().numpy(), out.status.cpu().numpy())
        else:
            o = qse.endpoint_batch_host(self._ep_state, self._state, slots, flags, tok, fs, enc, first, emit, blank, self.eplan)
        if int(o.status.max()) != 0:
            raise RuntimeError(f'stream: endpoint step refused, status {o.status.tolist()} for slots {slots}')
        self._ep_rows = {s: o.records[b, :int(o.n_records[b])].copy() for b, s in enumerate(slots)}

    def take_hits(self):
        """(spot=) the keyword hits that closed since the last call as qasr.ctc.StreamHit, sorted by (detected_s, slot, start_s,
        index); the queue is cleared"""
        if self.spot is None:
            raise ValueError('stream: take_hits needs a session opened with spot=')
        from qasr import stream_spot as qss
        out, self._hits = qss.sort_hits(self._hits), []
        return out

    def pending_hits(self, slot):
        """(spot=) the hits that are open after the last step of `slot`, one qasr.ctc.KeywordHit per keyword at most: what the
        stream shows now, before it is certain that nothing replaces it"""
        if self.spot is None:
            raise ValueError('stream: pending_hits needs a session opened with spot=')
        return list(self._pending.get(int(slot), []))

    def _spot(self, slots, end, sl, logp, enc, first, status, blank):
        """(spot=) k_star (penalty 0) and the spot launch (or their twins) behind a step's emit; queues the hits that closed and
        keeps the rows' open hits"""
        from qasr import align as qalign, engine as qengine, stream as qstream, stream_spot as qss
        B, K = len(slots), self.splan.K
        flags = [(qstream.END if end else 0) | (qstream.BEGIN if self._open[s]['spot_begin'] else 0) for s in slots]
        for s in slots:
            self._open[s]['spot_begin'] = False
        if self._dev.type == 'cuda':
            Tw = logp.shape[1]
            if self._sp_plane is None or self._sp_plane.shape[1] != Tw:
                self._sp_plane = torch.empty(self.S, Tw, device=self._dev, dtype=torch.float32)
            plane = qengine.ctc_star(logp, enc, 0.0, out=self._sp_plane[:B])
            out = qss.SpotStepBatch(*[getattr(self._sp_out, n)[:B * K] for n in qss.FIELDS])
            qengine.stream_spot(self._state, self._sp_state, self.S, self.plan, self.splan, sl, self._i32(flags), logp, plane, enc, first,
                                status, blank, keywords=self._sp_kw, out=out)
            o = qss.SpotStepBatch(*[getattr(out, n).cpu().numpy() for n in qss.FIELDS])
        else:
            o = qss.spot_batch_host(self._sp_state, self._state, slots, flags, logp, qalign.star_host(logp, enc, 0.0), enc, first, status,
                                    blank)
        if int(o.status.max()) != 0 or int(o.n_new_hits.max()) > o.hit_start.shape[1]:
            raise RuntimeError(f'stream: spot step refused, status {o.status.tolist()} / hits {o.n_new_hits.tolist()} for slots {slots}')
        final, pending = qss.to_stream_hits(o, slots, self._sp_given, self.plan.seconds_per_frame())
        self._hits += final
        self._pending.update(pending)

    def _step(self, slots, end):
        """one step for `slots`: window -> forward -> emit (-> endpoint) (-> star -> spot); returns the rows' deltas as
        qasr.stream.StepRow-like tuples"""
        from qasr import engine as qengine, stream as qstream
        m, plan, B = self.model, self.plan, len(slots)
        blank = len(m.decoder.vocabulary)
        flags = [qstream.END if end else 0] * B
        self.steps += 1
        if self._dev.type == 'cuda':
            sl, fl = self._i32(slots), self._i32(flags)
            win, wl, first = qengine.stream_window(self._state, self.S, plan, sl, out=tuple(t[:B] for t in self._win))
            if self.spot is not None:        # the spotter reads log-probabilities: the frame scores are gathered from them
                logp, enc, tok = m._forward(win, wl.long())
                logp = logp.float()
                tok = tok.to(torch.int32).contiguous()
                fs = m._frame_scores(logp, tok).contiguous()
            else:
                tok, fs, enc = m._forward(win, wl.long(), decode='frames')
                tok = tok.to(torch.int32).contiguous()
                fs = fs.float().contiguous()
            o = self._out
            fields = [f.name for f in dataclasses.fields(o)]
            out = qstream.StepBatch(*[None if getattr(o, n) is None else getattr(o, n)[:B] for n in fields])
            enc = enc.to(torch.int32).contiguous()
            qengine.stream_emit(self._state, self.S, plan, sl, fl, tok, fs, enc, first, blank, out=out)
            if self.endpoint is not None:
                self._endpoint(slots, end, sl, tok, fs, enc, first, out, blank)
            if self.spot is not None:
                self._spot(slots, end, sl, logp, enc, first, out.status, blank)
            o = qstream.StepBatch(*[None if getattr(out, n) is None else getattr(out, n).cpu().numpy() for n in fields])
        else:
            win, wl, first = qstream.window_host(self._state, slots)
            if self.spot is not None:
                logp, enc, tok = m._forward(torch.from_numpy(win), torch.from_numpy(wl).long())
                logp = logp.float()
                fs = m._frame_scores(logp, tok)
            else:
                tok, fs, enc = m._forward(torch.from_numpy(win), torch.from_numpy(wl).long(), decode='frames')
            o = qstream.emit_batch_host(self._state, slots, flags, tok.numpy(), fs.float().numpy(), enc.numpy(), first, blank)
            if self.endpoint is not None:
                self._endpoint(slots, end, None, tok.numpy(), fs.float().numpy(), enc.numpy(), first, o, blank)
            if self.spot is not None:
                self._spot(slots, end, None, logp.numpy(), enc.numpy(), first, o.status, blank)
            if not self.tail:
                o.tail_labels = o.tail_n = None
        if int(o.status.max()) != 0:
            raise RuntimeError(f'stream: step refused, status {o.status.tolist()} for slots {slots}')
        rows = []
        for b in range(B):
            n = int(o.n_new_labels[b])
            tl = o.tail_labels[b, :int(o.tail_n[b])].tolist() if o.tail_labels is not None else []
            rows.append((o.labels[b, :n].copy(), o.start[b, :n].copy(), o.nframes[b, :n].copy(), o.score[b, :n].copy(),
                         float(o.utt_score[b]), tl))
        return rows

    def _step_beam(self, slots, end):
        """one step of a beam session for `slots`: window -> forward with log-probabilities -> top-N -> beam -> emit (the
        greedy emit keeps the stream's counters); returns per row dict(labels, frames, tail, end, commit_len)"""
        from qasr import beam as qbeam, engine as qengine, stream as qstream, stream_beam as qsb
        m, plan, bp, bm, B = self.model, self.plan, self.bplan, self.beam, len(slots)
        blank = len(m.decoder.vocabulary)
        flags = [(qstream.END if end else 0) | (qstream.BEGIN if self._open[s]['beam_begin'] else 0) for s in slots]
        bset = [self._open[s]['boost_set'] for s in slots]     # read on BEGIN rows only
        for s in slots:
            self._open[s]['beam_begin'] = False
        self.steps += 1
        if self._dev.type == 'cuda':
            sl, fl = self._i32(slots), self._i32(flags)
            win, wl, first = qengine.stream_window(self._state, self.S, plan, sl, out=tuple(t[:B] for t in self._win))
            logp, enc, tok = m._forward(win, wl.long())
            logp = logp.float()
            tok = tok.to(torch.int32).contiguous()
            fs = m._frame_scores(logp, tok).contiguous()
            enc = enc.to(torch.int32).contiguous()
            Tw = logp.shape[1]
            if self._cand is None or self._cand[0].shape[1] != Tw:
                self._cand = tuple(torch.empty(self.S, Tw, bp.N, device=self._dev, dtype=torch.int32) for _ in range(2))
            cand = qengine.ctc_topn(logp, enc, bp.N, out=tuple(t[:B] for t in self._cand))
            names = [f.name for f in dataclasses.fields(self._bout)]
            bout = qsb.BeamStepBatch(*[None if getattr(self._bout, n) is None else getattr(self._bout, n)[:B] for n in names])
            if self._sets is None:
                qengine.stream_beam(self._state, self._bstate, self.S, plan, bp, sl, fl, cand[0], cand[1], enc, first, blank, bm.lm,
                                    bm.alpha, bm.beta, out=bout)
            else:
                qengine.stream_beam_boost(self._state, self._bstate, self.S, plan, bp, sl, fl, cand[0], cand[1], enc, first, blank,
                                          self._sets, self._i32(bset), bm.lm, bm.alpha, bm.beta, out=bout, blobs=self._set_blobs)
            fields = [f.name for f in dataclasses.fields(self._out)]
            eout = qstream.StepBatch(*[None if getattr(self._out, n) is None else getattr(self._out, n)[:B] for n in fields])
            qengine.stream_emit(self._state, self.S, plan, sl, fl, tok, fs, enc, first, blank, out=eout)
            o = qsb.BeamStepBatch(*[None if getattr(bout, n) is None else getattr(bout, n).cpu().numpy() for n in names])
            est = eout.status.cpu().numpy()
        else:
            win, wl, first = qstream.window_host(self._state, slots)
            logp, enc, tok = m._forward(torch.from_numpy(win), torch.from_numpy(wl).long())
            logp = logp.float()
            fs = m._frame_scores(logp, tok)
            cid, cq = qbeam.topn_host(logp.numpy(), bp.N, enc.numpy())
            o = qsb.step_batch_host(self._bstate, self._state, slots, flags, cid, cq, enc.numpy(), first, blank, bm.lm, bm.alpha, bm.beta,
                                    boost=self._sets, boost_set=bset if self._sets is not None else None)
            est = qstream.emit_batch_host(self._state, slots, flags, tok.numpy(), fs.numpy(), enc.numpy(), first, blank).status
        if int(o.status.max()) != 0 or int(est.max()) != 0:
            raise RuntimeError(f'stream: step refused, status {o.status.tolist()} / {est.tolist()} for slots {slots}')
        rows = []
        for b in range(B):
            n = int(o.n_new_labels[b])
            ends = [(o.end_labels[b, h, :int(o.end_n_labels[b, h])].tolist(), int(o.end_score[b, h]),
                     None if o.end_lm_score is None else int(o.end_lm_score[b, h]),
                     None if o.end_boost_score is None else int(o.end_boost_score[b, h])) for h in range(int(o.n_hyps[b]))]
            rows.append(dict(labels=o.labels[b, :n].copy(), frames=o.frames[b, :n].copy(), commit_len=int(o.commit_len[b]),
                             tail=o.tail_labels[b, :min(int(o.tail_n[b]), o.tail_labels.shape[1])].tolist(), end=ends))
        return rows

    def _step_beam_ep(self, slots, end):
        """one step of a beam session with StreamBeam(endpoint=) for `slots`: window -> forward with log-probabilities ->
        top-N -> emit -> endpoint -> beam (STREAM_BEAM_EP_RULES); the step's cuts become queued StreamUtterances; returns per
        row dict(labels, frames, tail, last) - last: the hypothesis (or n-best list) of the row's last cut, None without one"""
        from qasr import beam as qbeam, engine as qengine, stream as qstream, stream_beam as qsb, stream_ep as qse
        m, plan, bp, bm, B = self.model, self.plan, self.bplan, self.beam, len(slots)
        blank = len(m.decoder.vocabulary)
        flags = [(qstream.END if end else 0) | (qstream.BEGIN if self._open[s]['beam_begin'] else 0) for s in slots]
        bset = [self._open[s]['boost_set'] for s in slots]     # read on BEGIN rows only
        for s in slots:
            self._open[s]['beam_begin'] = self._open[s]['ep_begin'] = False
        self.steps += 1
        if self._dev.type == 'cuda':
            sl, fl = self._i32(slots), self._i32(flags)
            win, wl, first = qengine.stream_window(self._state, self.S, plan, sl, out=tuple(t[:B] for t in self._win))
            logp, enc, tok = m._forward(win, wl.long())
            logp = logp.float()
            tok = tok.to(torch.int32).contiguous()
            fs = m._frame_scores(logp, tok).contiguous()
            enc = enc.to(torch.int32).contiguous()
            Tw = logp.shape[1]
            if self._cand is None or self._cand[0].shape[1] != Tw:
                self._cand = tuple(torch.empty(self.S, Tw, bp.N, device=self._dev, dtype=torch.int32) for _ in range(2))
            cand = qengine.ctc_topn(logp, enc, bp.N, out=tuple(t[:B] for t in self._cand))
            fields = [f.name for f in dataclasses.fields(self._out)]
            eout = qstream.StepBatch(*[None if getattr(self._out, n) is None else getattr(self._out, n)[:B] for n in fields])
            qengine.stream_emit(self._state, self.S, plan, sl, fl, tok, fs, enc, first, blank, out=eout)
            pout = qse.EpStepBatch(*[getattr(self._ep_out, n)[:B] for n in ('records', 'n_records', 'status')])
            qengine.stream_endpoint(self._state, self._ep_state, self.S, plan, self.eplan, sl, fl, tok, fs, enc, first, eout, blank, out=pout)
            names = [f.name for f in dataclasses.fields(self._bout)]
            bout = qsb.BeamEpStepBatch(*[None if getattr(self._bout, n) is None else getattr(self._bout, n)[:B] for n in names])
            qengine.stream_beam_ep(self._state, self._bstate, self.S, plan, bp, sl, fl, cand[0], cand[1], enc, first, blank, pout,
                                   self._sets, self._i32(bset) if self._sets is not None else None, bm.lm, bm.alpha, bm.beta, out=bout,
                                   blobs=self._set_blobs if self._sets is not None else None)
            o = qsb.BeamEpStepBatch(*[None if getattr(bout, n) is None else getattr(bout, n).cpu().numpy() for n in names])
            est, recs, pst = eout.status.cpu().numpy(), pout.records.cpu().numpy(), pout.status.cpu().numpy()
        else:
            win, wl, first = qstream.window_host(self._state, slots)
            logp, enc, tok = m._forward(torch.from_numpy(win), torch.from_numpy(wl).long())
            logp = logp.float()
            fs = m._frame_scores(logp, tok)
            cid, cq = qbeam.topn_host(logp.numpy(), bp.N, enc.numpy())
            eo = qstream.emit_batch_host(self._state, slots, flags, tok.numpy(), fs.numpy(), enc.numpy(), first, blank)
            po = qse.endpoint_batch_host(self._ep_state, self._state, slots, flags, tok.numpy(), fs.numpy(), enc.numpy(), first, eo, blank,
                                         self.eplan)
            o = qsb.step_batch_ep_host(self._bstate, self._state, slots, flags, cid, cq, enc.numpy(), first, po.records, po.n_records,
                                       po.status, blank, bm.lm, bm.alpha, bm.beta, boost=self._sets,
                                       boost_set=bset if self._sets is not None else None)
            est, recs, pst = eo.status, po.records, po.status
        if int(o.status.max()) != 0 or int(est.max()) != 0 or int(pst.max()) != 0:
            raise RuntimeError(f'stream: step refused, status {o.status.tolist()} / {est.tolist()} / {pst.tolist()} for slots {slots}')
        rows = []
        for b, s in enumerate(slots):
            n = int(o.n_new_labels[b])
            lab, fr = o.labels[b, :n].copy(), o.frames[b, :n].copy()
            rows.append(dict(labels=lab, frames=fr, tail=o.tail_labels[b, :min(int(o.tail_n[b]), o.tail_labels.shape[1])].tolist(),
                             last=self._cut_beam(s, o, b, recs[b], lab, fr)))
        return rows

    def _cut_beam(self, slot, o, b, recs, lab, fr):
        """(StreamBeam(endpoint=)) the cuts of row b of a step: each takes the utterance's labels - what the slot's open
        utterance had committed, and the step's delta up to cut_delta_end - and becomes a queued StreamUtterance whose
        hypothesis is the beam's best; the delta behind the last cut stays with the slot.  Returns the last cut's hypothesis
        (the list with n_best > 1), None without a cut."""
        from qasr import beam as qbeam, ctc as qctc, stream_ep as qse
        st, last, at = self._open[slot], None, 0
        vocab, spf_s = self.model.decoder.vocabulary, self.plan.seconds_per_frame()
        text = lambda ids: ''.join(vocab[i] for i in ids)
        for k in range(int(o.n_cuts[b])):
            de, r = int(o.cut_delta_end[b, k]), recs[k]
            ul = np.concatenate([d[0] for d in st['deltas']] + [lab[at:de]]).astype(np.int32).tolist()
            uf = np.concatenate([d[1] for d in st['deltas']] + [fr[at:de]]).astype(np.float64)
            st['deltas'], at = [], de
            hyps = []
            for h in range(int(o.cut_n_hyps[b, k])):
                labs = ul[:len(ul) - int(o.cut_n_labels[b, k, 0])] + o.cut_labels[b, k, h, :int(o.cut_n_labels[b, k, h])].tolist()
                hyp = qctc.Hypothesis(text(labs), labs, (uf * spf_s).tolist() if h == 0 else [], ((uf + 1) * spf_s).tolist() if h == 0 else [],
                                      None, None, [])
                hyp.utt_score = float(o.cut_score[b, k, h]) / qbeam.ONE
                if o.cut_lm_score is not None:
                    hyp.lm_score = float(o.cut_lm_score[b, k, h]) / qbeam.ONE
                if o.cut_boost_score is not None:
                    hyp.boost_score = float(o.cut_boost_score[b, k, h]) / qbeam.ONE
                hyps.append(hyp)
            if not hyps:                     # the beam had died: the committed text of the utterance alone
                hyps = [qctc.Hypothesis(text(ul), ul, (uf * spf_s).tolist(), ((uf + 1) * spf_s).tolist(), None, None, [])]
            sp = int(r[qse.R_SP_FIRST]) >= 0
            utt = qctc.StreamUtterance(slot, int(r[qse.R_INDEX]), qse.REASONS[int(r[qse.R_REASON])], int(r[qse.R_FIRST]) * spf_s,
                                       int(r[qse.R_END]) * spf_s, int(r[qse.R_SP_FIRST]) * spf_s if sp else None,
                                       (int(r[qse.R_SP_LAST]) + 1) * spf_s if sp else None, hyps[0])
            if self.beam.n_best > 1:
                utt.n_best = hyps
            self._utts.append(utt)
            last = hyps if self.beam.n_best > 1 else hyps[0]
        if len(lab) > at:
            st['deltas'].append((lab[at:], fr[at:]))
        return last

    def _close_beam(self, st, slot):
        """the END step of a beam session: committed text + the remainder of each of the n_best final entries"""
        from qasr import beam as qbeam, ctc as qctc
        vocab, spf_s = self.model.decoder.vocabulary, self.plan.seconds_per_frame()
        if self.endpoint is not None:        # the END utterance: the END record's cut
            try:
                if st['received'] > 0:
                    return self._step_beam_ep([slot], True)[0]['last']
                # a stream that never received a sample has nothing to run: the empty END utterance
                hyp = qctc.Hypothesis('', [], [], [], None, None, [])
                hyp.utt_score = 0.0
                if self.beam.lm is not None:
                    hyp.lm_score = 0.0
                if self._sets is not None:
                    hyp.boost_score = 0.0
                utt = qctc.StreamUtterance(slot, 0, 'end', 0.0, 0.0, None, None, hyp)
                if self.beam.n_best > 1:
                    utt.n_best = [hyp]
                self._utts.append(utt)
                return [hyp] if self.beam.n_best > 1 else hyp
            finally:
                self._open.pop(slot)
        ends = []
        try:
            if st['received'] > 0:
                row = self._step_beam([slot], True)[0]
                st['deltas'].append((row['labels'], row['frames']))
                ends = row['end']
        finally:
            self._open.pop(slot)
        lab = np.concatenate([d[0] for d in st['deltas']] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
        fr = np.concatenate([d[1] for d in st['deltas']] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
        text = lambda ids: ''.join(vocab[i] for i in ids)
        best = qctc.Hypothesis(text(lab.tolist()), lab.tolist(), (fr.astype(np.float64) * spf_s).tolist(),
                               ((fr + 1).astype(np.float64) * spf_s).tolist(), None, None, [])
        head = lab.tolist()[:len(lab) - len(ends[0][0])] if ends else lab.tolist()
        hyps = []
        for h, (suffix, sc, lmt, bt) in enumerate(ends):
            hyp = best if h == 0 else qctc.Hypothesis(text(head + suffix), head + suffix, [], [], None, None, [])
            hyp.utt_score = float(sc) / qbeam.ONE
            if lmt is not None:
                hyp.lm_score = float(lmt) / qbeam.ONE
            if bt is not None:
                hyp.boost_score = float(bt) / qbeam.ONE
            hyps.append(hyp)
        if not hyps:                         # nothing was received, or the beam died: the committed text alone
            hyps = [best]
        return hyps if self.beam.n_best > 1 else hyps[0]

    def push(self, slots, signal, lengths=None):
        """signal [B, n] float32 or int16 at the model's rate, lengths [B] (default: n each), slots: B distinct open slots.
        A session opened with input_rate= takes [B, n * channels] interleaved PCM at that rate, lengths in frames; a slot
        keeps the sample format of its first push.  Returns the StreamUpdates of the steps this audio completed, in the
        order they ran."""
        from qasr import stream as qstream
        slots = [int(s) for s in (slots.tolist() if torch.is_tensor(slots) else slots)]
        if signal.dim() != 2 or signal.shape[0] != len(slots) or signal.dtype not in (torch.float32, torch.int16):
            raise ValueError(f'stream: signal must be float32 or int16 [{len(slots)}, n], got {signal.dtype} {tuple(signal.shape)}')
        if len(set(slots)) != len(slots) or any(s not in self._open for s in slots):
            raise ValueError(f'stream: slots {slots} must be distinct and open (open slots: {sorted(self._open)})')
        if self.rs_plan is not None:
            return self._push_resampled(slots, signal, lengths)
        lens = [signal.shape[1]] * len(slots) if lengths is None else [int(x) for x in torch.as_tensor(lengths).tolist()]
        if len(lens) != len(slots) or any(not 0 <= n <= signal.shape[1] for n in lens):
            raise ValueError(f'stream: lengths {lens} must be one per slot, each within 0 .. {signal.shape[1]}')
        self._setup(signal.device)
        C = self.plan.C
        pieces = [qstream.split_pushes(self._open[s]['received'] % C, n, C) for s, n in zip(slots, lens)]
        offs = [0] * len(slots)
        updates = []
        for k in range(max([len(p) for p in pieces] + [0])):
            rows = [i for i in range(len(slots)) if k < len(pieces[i])]
            n_new = [pieces[i][k] for i in rows]
            w = max(n_new)
            chunk = torch.zeros(len(rows), w, dtype=signal.dtype, device=signal.device)
            for j, i in enumerate(rows):
                chunk[j, :n_new[j]] = signal[i, offs[i]:offs[i] + n_new[j]]
                offs[i] += n_new[j]
            sl = [slots[i] for i in rows]
            self._push(sl, [qstream.BEGIN if self._open[s]['begin'] else 0 for s in sl], n_new, chunk)
            stepping = []
            for s, n in zip(sl, n_new):
                st = self._open[s]
                st['begin'] = False
                st['received'] += n
                if st['received'] % C == 0:
                    stepping.append(s)
            if stepping:
                updates += self._updates(stepping)
        return updates

    def close(self, slot):
        """The END step of one stream: every frame of its last window becomes final.  Returns its qasr.ctc.Hypothesis; the
        slot is free again."""
        from qasr import ctc as qctc
        slot = int(slot)
        if slot not in self._open:
            raise ValueError(f'stream: slot {slot} is not open (open slots: {sorted(self._open)})')
        st = self._open[slot]
        self.closing_updates = []
        if self.rs_plan is not None and st['in_received'] > 0:     # the filter's tail: FLUSH rounds, stepping when a chunk fills
            zero = torch.zeros(1, self.rs_plan.channels, dtype=st['fmt'], device=self._dev)
            self.closing_updates = self._rounds_rs([slot], [0], zero, flush=True)
        if self.beam is not None:
            return self._close_beam(st, slot)
        if self.endpoint is not None:        # the END utterance: what is left of the stream behind its last cut
            from qasr import stream_ep as qse
            try:
                if st['received'] > 0:
                    lab, start, nfr, sc, utt, _ = self._step([slot], True)[0]
                    st['deltas'].append((lab, start, nfr, sc))
                    return self._cut(slot)
                # a stream that never received a sample has nothing to run: the END record of a fresh block
                return self._cut(slot, [qse._record(0, 0, 0, 0, 0, 0, qse.UTT_END, np.float32(0), 0)])
            finally:
                self._open.pop(slot)
        utt = 0.0
        try:
            if st['received'] > 0:           # (a stream that never received a sample has nothing to run)
                lab, start, nfr, sc, utt, _ = self._step([slot], True)[0]
                st['deltas'].append((lab, start, nfr, sc))
        finally:
            self._open.pop(slot)
        cat = lambda i, dt: np.concatenate([d[i] for d in st['deltas']] + [np.zeros(0, dtype=dt)]).astype(dt)[None]
        lab = cat(0, np.int32)
        res = qctc.CtcResult(lab, np.array([lab.shape[1]], dtype=np.int32), cat(1, np.int32), cat(2, np.int32), cat(3, np.float32),
                             np.array([utt], dtype=np.float32), len(self.model.decoder.vocabulary))
        return qctc.to_hypotheses(res, self.model.decoder.vocabulary, self.plan.seconds_per_frame())[0]
