"""GPU tests of the drop-in surface: HIP mel front-end, EncDecCTCModel in engine mode, the CLI."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import nemo.quantization.utils.quantize_model as qm  # noqa: E402
from nemo.collections.asr.models import EncDecCTCModel  # noqa: E402
from qasr import configs, synth, topology  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.set_grad_enabled(False)


def test_frontend_hip_matches_reference(golden_dir):
    """qasr_frontend_mel vs FilterbankFeatures of the reference (fixture), tolerance-based: <= 1e-4 absolute on the
    normalised log-mel.  The spectrum is computed in float64 and rounded once; an exact spectrum
    followed by the reference's float32 steps sits at 5.5e-5 max / 4e-7 mean from the fixture (the reference's own
    float32 FFT rounding), which is what this kernel should reproduce."""
    from qasr import engine
    d = np.load(os.path.join(golden_dir, 'frontend.npz'))
    y, seq = engine.frontend_mel(torch.from_numpy(d['audio']).cuda(), torch.from_numpy(d['lens']).cuda(),
                                 torch.from_numpy(d['fb']), torch.from_numpy(d['window']), 0.97, 16)
    assert np.array_equal(seq.cpu().numpy(), d['seq_len'])
    y = y.cpu().numpy()
    assert y.shape == d['feats'].shape
    err = np.abs(y - d['feats'])
    assert err.max() <= 1e-4, err.max()
    assert err.mean() < 2e-6, err.mean()
    for b, n in enumerate(d['seq_len']):
        assert np.all(y[b, :, n:] == 0)          # masked + pad_to frames are exactly zero


def test_frontend_planned_equals_self_contained(golden_dir):
    """qasr_frontend_plan + qasr_frontend_mel_planned (what a model with a fixed filterbank calls per batch) is the same
    computation as the self-contained qasr_frontend_mel: bit-identical features; and a filterbank too large for the
    LDS table (here: more filters than MEL_MAXM) takes the global-memory projection with the same result per filter."""
    from qasr import engine
    d = np.load(os.path.join(golden_dir, 'frontend.npz'))
    audio, lens = torch.from_numpy(d['audio']).cuda(), torch.from_numpy(d['lens']).cuda()
    fb, win = torch.from_numpy(d['fb']).cuda().contiguous(), torch.from_numpy(d['window']).cuda()
    y0, s0 = engine.frontend_mel(audio, lens, fb, win, 0.97, 16)
    plan = engine.frontend_plan(fb)
    for _ in range(2):                                         # the plan is read-only: reusable
        y1, s1 = engine.frontend_mel(audio, lens, fb, win, 0.97, 16, plan=plan)
        assert torch.equal(y0, y1) and torch.equal(s0, s1)
    big = torch.cat([fb, fb, fb.flip(0)[:8]]).contiguous()     # 136 filters > MEL_MAXM: read from global memory
    yb, _ = engine.frontend_mel(audio, lens, big, win, 0.97, 16)
    n = fb.shape[0]
    assert torch.equal(yb[:, :n], y0) and torch.equal(yb[:, n:2 * n], y0)
    assert torch.equal(yb[:, 2 * n:], y0.flip(1)[:, :8])


def _prepared_model(name='MiniQuartzNet', seed=1, wbit=8, abit=8, percentile=None, feat=16, frames=96):
    m = EncDecCTCModel.from_synthetic(name, seed=seed).cuda()
    m.eval()
    m.set_quant_bit(wbit, mode='weight')
    m.set_quant_bit(abit, mode='act')
    if percentile is not None:
        qm.set_percentile(m, percentile)
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([frames] * 4).cuda()
    for c in synth.make_calibration(3, 4, feat, frames, seed):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    return m


@pytest.mark.parametrize('name,wbit,abit,pct', [('MiniQuartzNet', 8, 8, None), ('MiniQuartzNet', 6, 6, 99.9),
                                                ('MiniJasper', 8, 8, None)])
def test_model_engine_path_equals_host_path(name, wbit, abit, pct):
    """EncDecCTCModel.forward (HIP engine) vs the same calibrated modules run by host PyTorch."""
    m = _prepared_model(name, seed=2, wbit=wbit, abit=abit, percentile=pct)
    assert m.engine_ready()
    x = torch.from_numpy(synth.make_features(5, 16, 96, 7)).cuda()
    lens = torch.tensor([96, 90, 61, 33, 12]).cuda()
    lp, el, tok = m(processed_signal=x, processed_signal_length=lens)
    e, l, sf = m.encoder(audio_signal=x, length=lens)
    lp_host = m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    assert torch.equal(el, l)
    assert torch.equal(tok, lp_host.argmax(-1))
    np.testing.assert_allclose(lp.cpu().numpy(), lp_host.cpu().numpy(), rtol=1e-4, atol=2e-5)
    assert tok.dtype == torch.int64 and lp.shape == (5, 48, 29)


def test_model_from_audio_full_quartznet():
    """Audio -> HIP front-end -> integer QuartzNet15x5 -> tokens, against host front-end + host modules.
    The two front-ends differ by float rounding (<= 1e-4 on the features), so a few first-layer roundings may flip:
    tokens must agree on >= 99 % of frames of this random-weight net, whose argmax margins are tiny (bit-exactness is
    defined from identical features, SURVEY hard-part 6, and checked at the end of this test)."""
    m = _prepared_model('QuartzNet15x5Base-En', seed=5, percentile=99.996, feat=64, frames=128)
    m.preprocessor.featurizer.dither = 0.0
    audio = torch.from_numpy(synth.make_audio(4, 32000, seed=3)).cuda()
    alen = torch.tensor([32000, 30000, 20011, 16000]).cuda()
    for i, n in enumerate(alen.tolist()):
        audio[i, n:] = 0
    lp, el, tok = m(input_signal=audio, input_signal_length=alen)
    feats, flen = m.preprocessor(input_signal=audio, length=alen)
    e, l, sf = m.encoder(audio_signal=feats, length=flen)
    tok_host = m.decoder(encoder_output=e, encoder_output_scaling_factor=sf).argmax(-1)
    assert torch.equal(el, l)
    agree = (tok == tok_host).float().mean().item()
    assert agree >= 0.99, agree
    # identical features -> identical tokens (the bit-exact contract)
    lp2, _, tok2 = m(processed_signal=feats, processed_signal_length=flen)
    assert torch.equal(tok2, tok_host)


def _write_wav(path, x):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype('<i2').tobytes())


def _cli(tmp_path, extra, n_utt, samples, seed, text):
    """Runs examples/asr/quantization/inference.py on synthetic WAVs (no dataset / checkpoint ships); returns the
    manifest path, its stdout and the --dump_hyps record."""
    man = tmp_path / 'manifest.json'
    audio = synth.make_audio(n_utt, samples, seed=seed)
    with open(man, 'w') as f:
        for i in range(n_utt):
            p = str(tmp_path / f'u{i}.wav')
            n = samples - 1000 * i
            _write_wav(p, audio[i, :n])
            f.write(json.dumps(dict(audio_filepath=p, duration=n / 16000, text=text)) + '\n')
    cli = os.path.join(ROOT, 'q-asr_amd', 'examples', 'asr', 'quantization', 'inference.py')
    dump = tmp_path / 'hyps.json'
    out = subprocess.run([sys.executable, cli, '--asr_model', 'QuartzNet15x5Base-En', '--synthetic_model', '--dataset', str(man),
                          '--weight_bit', '8', '--act_bit', '8', '--dither', '0', '--dump_hyps', str(dump)] + extra,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump) as f:
        return str(man), out.stdout, json.load(f)


def _expected_hypotheses(m, manifest, batch_size):
    """What the CLI must print for `manifest`, computed WITHOUT EncDecCTCModel.forward's engine routing: (a) the HIP front-end's
    features through the calibrated HOST modules (encoder + decoder in PyTorch: identical features -> identical integers ->
    identical hypotheses) and (b) the host front-end in front of the same modules (features within 1e-4: nearly all characters)."""
    from nemo.collections.asr.metrics.wer import WER, word_error_rate
    m.preprocessor.featurizer.dither = 0.0
    m.setup_test_data(test_data_config={'sample_rate': 16000, 'manifest_filepath': manifest, 'labels': m.decoder.vocabulary,
                                        'batch_size': batch_size, 'normalize_transcripts': True, 'shuffle': False})
    wer = WER(vocabulary=m.decoder.vocabulary)
    labels_map = dict(enumerate(m.decoder.vocabulary))
    hyps, hyps_host, refs = [], [], []
    for batch in m.test_dataloader():
        sig, n = batch[0].cuda().float(), batch[1].cuda()
        for front, acc in ((m._frontend_hip, hyps), (lambda s, l: m.preprocessor(input_signal=s, length=l), hyps_host)):
            feats, flen = front(sig, n)
            e, _, sf = m.encoder(audio_signal=feats, length=flen)
            acc += wer.ctc_decoder_predictions_tensor(m.decoder(encoder_output=e, encoder_output_scaling_factor=sf).argmax(-1))
        refs += [''.join(labels_map[c] for c in row) for row in batch[2].cpu().numpy()]
    return hyps, hyps_host, refs, word_error_rate(hypotheses=hyps, references=refs)


def _char_agreement(a, b):
    import difflib
    return min(difflib.SequenceMatcher(None, x, y).ratio() for x, y in zip(a, b))


def test_cli_inference_runs(tmp_path):
    """examples/asr/quantization/inference.py end to end (inference.py:145-159): the hypotheses and the WER it reports equal
    what the host modules decode from the same WAVs with the same calibration."""
    man, stdout, rec = _cli(tmp_path, ['--batch_size', '3', '--synthetic_calib', '2', '--percentile', '99.996'], 6, 24000, 1,
                            'hello world')
    assert 'RTFx' in stdout and 'path: static integer engine (HIP)' in stdout and rec['path'] == 'Engine'
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En').cuda()
    m.eval()
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    qm.set_percentile(m, 99.996)
    m.encoder.bn_folding()
    qm.calibrate(m)
    L = torch.tensor([500] * 3).cuda()
    for c in synth.make_calibration(2, 3, 64, 500):
        e, _, sf = m.encoder(audio_signal=torch.from_numpy(c).cuda(), length=L)
        m.decoder(encoder_output=e, encoder_output_scaling_factor=sf)
    qm.evaluate(m)
    qm.set_dynamic(m, False)
    hyps, hyps_host, refs, wer_value = _expected_hypotheses(m, man, 3)
    assert len(rec['hypotheses']) == 6 and all(len(h) > 0 for h in hyps)           # a random-weight net still emits characters
    assert rec['references'] == refs == ['hello world'] * 6
    assert rec['hypotheses'] == hyps
    assert rec['wer'] == wer_value and f'WER: {wer_value}' in stdout
    assert _char_agreement(rec['hypotheses'], hyps_host) >= 0.9


def test_cli_inference_dynamic(tmp_path):
    """BASELINE.json config 1: inference.py --dynamic, batch size 1 (no calibration data): the dynamic-quantisation
    device path (qasr.dynamic) serves the forward passes; its hypotheses / WER equal what the CPU oracle's dynamic mode
    (quant_modules.py:149-167; pinned by the reference's own dynamic fixtures) decodes from the same features."""
    from nemo.collections.asr.metrics.wer import WER, word_error_rate
    from oracle import int_oracle as O
    man, stdout, rec = _cli(tmp_path, ['--batch_size', '1', '--dynamic'], 2, 20000, 2, 'a b')
    assert 'path: dynamic device path (HIP)' in stdout and rec['path'] == 'DynamicRunner'
    m = EncDecCTCModel.from_synthetic('QuartzNet15x5Base-En').cuda()
    m.eval()
    m.set_quant_bit(8, mode='weight')
    m.set_quant_bit(8, mode='act')
    m.encoder.bn_folding()
    qm.evaluate(m)
    qm.set_dynamic(m, True)
    _, hyps_host, refs, _ = _expected_hypotheses(m, man, 1)
    cfg = topology.quartznet15x5()
    net = O.OracleNet(topology.conv_plan(cfg), cfg, synth.make_state_dict(cfg, 0), None, None, 8, 8, dynamic=True,
                      division_residue=True)
    wer = WER(vocabulary=m.decoder.vocabulary)
    hyps = []
    for batch in m.test_dataloader():
        feats, flen = m._frontend_hip(batch[0].cuda().float(), batch[1].cuda())
        want = net.forward(feats.cpu().numpy(), [int(flen[0])])
        hyps += wer.ctc_decoder_predictions_tensor(torch.from_numpy(np.asarray(want['tokens'])).long())
    assert rec['references'] == refs == ['a b'] * 2
    assert all(len(h) > 0 for h in hyps) and rec['hypotheses'] == hyps
    wer_value = word_error_rate(hypotheses=hyps, references=refs)
    assert rec['wer'] == wer_value and f'WER: {wer_value}' in stdout
    # host modules on the GPU in dynamic mode: every range depends on PyTorch-ROCm's float division / min / max of the whole
    # tensor and this random-weight net has tiny argmax margins (measured 0.8): a plausibility bound, the oracle is the check
    assert _char_agreement(rec['hypotheses'], hyps_host) >= 0.6


@pytest.mark.parametrize('fuse_norm,S', [(True, 40000), (False, 40000), (True, 100000)])
def test_forward_audio_equals_frontend_plus_forward(golden_dir, fuse_norm, S):
    """qasr_engine_forward_audio (front-end inside the engine call, one hipGraph launch per batch) against
    qasr_frontend_mel followed by qasr_engine_forward: identical features, log-probs, tokens and lengths - on the direct
    launches of the first call, on the capture and on the replays.  fuse_norm (the default): normalize_batch runs inside
    k_stem from k_mel's per-tile float64 sums, one launch fewer; `feats` then holds the log-mel before normalisation and
    everything behind it must still be identical (ragged lengths down to 3 frames, a length that ends inside a tile; 100000
    samples = 40 statistics tiles, more than a thread of k_stem keeps in registers)."""
    from qasr import engine, pack
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5()
    sd = synth.make_state_dict(cfg, meta['seed'])
    blob, _ = pack.pack_model(cfg, sd, d['act_min'], d['act_max'], 8, 8)
    from qasr import melbank
    fb = torch.from_numpy(melbank.mel_filterbank(16000, 512, 64, 0.0, 8000.0).astype(np.float32)).cuda().contiguous()
    win = torch.hann_window(320, periodic=False).cuda()
    B = 4
    audio = torch.from_numpy(synth.make_audio(B, S, seed=5)).cuda()
    alen = torch.tensor([S, S - 7001, S - 16000, 400], dtype=torch.int32).cuda()
    e1, e2 = engine.Engine(blob, 0, graph=True), engine.Engine(blob, 0, graph=True, fuse_norm=fuse_norm)
    assert e2.opts.fuse_norm == int(fuse_norm)
    feats, flen = engine.frontend_mel(audio, alen, fb, win, 0.97, 16)
    lp0, tk0, el0 = e1.forward(feats, flen)
    plan = engine.frontend_plan(fb)
    st = torch.cuda.Stream()
    fbuf = torch.empty_like(feats)
    lbuf = torch.empty(B, dtype=torch.int32, device='cuda')
    out = (torch.empty_like(lp0), torch.empty_like(tk0), torch.empty_like(el0))
    torch.cuda.synchronize()
    for call in range(4):                                      # direct, capture, replay, replay
        for t in out:
            t.zero_()
        fbuf.zero_()
        with torch.cuda.stream(st):
            lp, tk, el = e2.forward_audio(audio, alen, fb, win, plan, 0.97, 16, feats=fbuf, feat_lens=lbuf, out=out)
        torch.cuda.synchronize()
        assert torch.equal(lbuf, flen), call
        if fuse_norm:                                            # un-normalised log-mel: normalising it here gives the features
            for b_ in range(B):
                n = int(flen[b_])
                x = fbuf[b_, :, :n].double()
                want = (x - x.mean(1, keepdim=True).float().double()) / (x.std(1, keepdim=True).float().double() + 1e-5)
                torch.testing.assert_close(want.float(), feats[b_, :, :n], rtol=1e-5, atol=1e-5)
        else:
            assert torch.equal(fbuf, feats), call
        assert torch.equal(lp, lp0) and torch.equal(tk, tk0) and torch.equal(el, el0), call
    assert e2.num_launches() == e1.num_launches() + (1 if fuse_norm else 2), (e1.num_launches(), e2.num_launches())
    # a larger batch through the same engine: new plan, larger statistics buffer, the old graph must not be replayed
    audio2, alen2 = torch.cat([audio, audio.flip(0)]).contiguous(), torch.cat([alen, alen.flip(0)]).contiguous()
    for call in range(3):
        with torch.cuda.stream(st):
            lp2, tk2, el2 = e2.forward_audio(audio2, alen2, fb, win, plan, 0.97, 16)
        torch.cuda.synchronize()
        assert torch.equal(tk2[:B], tk0) and torch.equal(tk2[B:], tk0.flip(0)) and torch.equal(el2[:B], el0), call
        assert torch.equal(lp2[:B], lp0), call
    e1.close()
    e2.close()


def test_graph_key_covers_frontend_arguments(golden_dir):
    """the captured front-end nodes bake in S, the filterbank and the window.  Two sample counts with the same
    padded frame count (40000 and 39840 samples -> 251 / 250 frames -> T_pad 256) through the SAME buffers, and a swapped
    filterbank pointer, must not replay the old graph: every call equals the kernel-by-kernel engine."""
    from qasr import engine, melbank, pack
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5()
    sd = synth.make_state_dict(cfg, meta['seed'])
    blob, _ = pack.pack_model(cfg, sd, d['act_min'], d['act_max'], 8, 8)
    fb = torch.from_numpy(melbank.mel_filterbank(16000, 512, 64, 0.0, 8000.0).astype(np.float32)).cuda().contiguous()
    fb2 = (fb * 0.5).contiguous()                              # another filterbank (own tables, own pointer)
    win = torch.hann_window(320, periodic=False).cuda()
    plan, plan2 = engine.frontend_plan(fb), engine.frontend_plan(fb2)
    B = 3
    base = torch.empty(B * 40000, device='cuda')
    g, ref = engine.Engine(blob, 0, graph=True), engine.Engine(blob, 0)
    T_pad = g.lib.qasr_frontend_frames(40000, 16)
    assert T_pad == g.lib.qasr_frontend_frames(39840, 16) == 256
    To = g.out_frames(T_pad)
    fbuf = torch.empty(B, 64, T_pad, device='cuda')
    lbuf = torch.empty(B, dtype=torch.int32, device='cuda')
    out = (torch.empty(B, To, 29, device='cuda'), torch.empty(B, To, dtype=torch.int32, device='cuda'),
           torch.empty(B, dtype=torch.int32, device='cuda'))
    st = torch.cuda.Stream()
    calls = [(40000, fb, plan)] * 3 + [(39840, fb, plan)] * 3 + [(39840, fb2, plan2)] * 3 + [(40000, fb, plan)] * 2
    for ci, (S, f, pl) in enumerate(calls):
        audio = base[:B * S].view(B, S)
        audio.copy_(torch.from_numpy(synth.make_audio(B, S, seed=50 + S % 7)))
        alen = torch.tensor([S, S - 4000, S - 9000], dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        lp0, tk0, el0 = ref.forward_audio(audio, alen, f, win, pl, 0.97, 16)
        for t in out:
            t.zero_()
        with torch.cuda.stream(st):
            lp, tk, el = g.forward_audio(audio, alen, f, win, pl, 0.97, 16, feats=fbuf, feat_lens=lbuf, out=out)
        torch.cuda.synchronize()
        assert torch.equal(tk, tk0) and torch.equal(el, el0) and torch.equal(lp, lp0), (ci, S)
    g.close()
    ref.close()


def test_distill_on_gpu_matches_reference_fixture(golden_dir):
    """SURVEY 8f-3 on PyTorch-ROCm: get_synthetic_data with the model on the GPU against tests/golden/distill.npz (the
    reference's own module on the CPU, 3 Adam iterations from a fixed start).  Tolerance: MIOpen's float32 conv / reduction
    order differs from the CPU's - losses rtol 1e-3, refined batches atol 2e-3 (the data moves by up to 0.15; Adam's first
    steps are sign-like, so a step flips only where a gradient is within rounding of zero)."""
    from nemo.collections.asr.models import EncDecCTCModel
    from nemo.quantization.utils import distill_data
    d = np.load(os.path.join(golden_dir, 'distill.npz'))
    meta = json.loads(str(d['meta']))
    m = EncDecCTCModel.from_synthetic(meta['model'], seed=meta['seed']).cuda()
    m.set_quant_mode('none')
    hist = []
    out = distill_data.get_synthetic_data(m.encoder, m.decoder, batch_size=meta['batch'], dim=d['start'].shape[2], seqlen=meta['frames'],
                                          train_iter=meta['train_iter'], num_batch=meta['num_batch'], lr=meta['lr'], verbose=False,
                                          history=hist, init=[torch.from_numpy(t) for t in d['start']])
    assert all(t.is_cuda for t in out)
    np.testing.assert_allclose(np.array(hist), d['losses'], rtol=1e-3)
    got = np.stack([t.cpu().numpy() for t in out])
    assert np.mean(np.abs(got - d['refined']) <= 2e-3) > 0.999, float(np.abs(got - d['refined']).max())


def test_bench_exchange_steps_on_a_one_rank_rccl_communicator():
    """The N-GPU exchange steps of bench.py (blob broadcast, per-step token gather to rank 0, max-over-ranks
    all-reduce, rank census) executed through torch.distributed's "nccl" backend = RCCL on the one GPU of this box
    (QASR_BENCH_FORCE_DIST=1: a communicator of one rank makes the same calls, on the device, as the 8-rank run)."""
    env = dict(os.environ, QASR_BENCH_FORCE_DIST='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29541')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '8', '--warmup', '2',
                          '--full', '--no-cpu-baseline'], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line['n_gpus'] == 1 and line['n_ranks_seen'] == 1 and line['steps'] == 8
    assert 'RCCL blob broadcast + token gather' in line['config']['parallelism']
    assert line['value'] > 0


@pytest.mark.parametrize('gather', ['tokens', 'logits'])
def test_bench_two_ranks_with_real_engines_gloo_rehearsal(gather):
    """The N > 1 bench loop with REAL engines and 4 steps in flight per rank, two ranks (both on GPU 0 - the box has one -
    exchange steps through gloo / host memory: QASR_BENCH_BACKEND=gloo).  A FRESH child process runs torch.distributed.run,
    which spawns its ranks before anything touches the GPU.  Checked: both ranks counted, rank 1 built its engines from the
    broadcast blob (equal digests; the receiving rank also ran qasr_blob_check), rank 0's slot of every stream's receive
    buffers equals its local result, and what the gather delivered FROM RANK 1 equals rank 0's own recomputation of rank 1's
    steps (rank 1's audio seeds) - tokens, and with --gather logits the float32 log-probs (north_star's wording)."""
    env = dict(os.environ, QASR_BENCH_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'QASR_BENCH_FORCE_DIST'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                          '127.0.0.1', '--master-port', '29547' if gather == 'tokens' else '29549', os.path.join(ROOT, 'bench.py'),
                          '--gpus', '2', '--steps', '8', '--warmup', '2', '--full', '--no-cpu-baseline', '--gather', gather, '--check-gather'],
                         capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.strip().splitlines() if l.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['n_ranks_seen'] == 2 and line['steps'] == 8
    assert line['blob_digests_equal_across_ranks'] is True
    assert line['gather_checked_ranks'] == [1]
    assert line['config']['global_batch'] == 64 and line['config']['steps_in_flight'] == 4
    assert ('logits gather' if gather == 'logits' else 'token gather') in line['config']['parallelism']
    assert line['value'] > 0


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    """A plain bench run (no --full) times exactly --steps steps, prints the headline without the --full figures, and
    --dump-outputs writes what the last timed step returned.  This process rebuilds the same model, runs the same seeded audio
    batch (step K - 1 ran on stream (K - 1) % S) through a fresh engine and compares: tokens and encoded lengths bit for bit,
    the log-probs (written with --gather logits) to float rounding."""
    import bench
    from qasr import engine
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'QASR_BENCH_FORCE_DIST'):
        env.pop(k, None)
    steps, dump = 7, tmp_path / 'outputs'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2',
                          '--gather', 'logits', '--dump-outputs', str(dump)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line['steps'] == steps and line['ms_per_step'] > 0
    assert abs(line['value'] - 32 * 5.0 / (line['ms_per_step'] * 1e-3)) / line['value'] < 1e-6
    assert not {'roofline', 'cpu_baseline', 'other_configs', 'single_stream_ms_per_step'} & set(line), sorted(line)
    got = {n: np.load(dump / f'{n}.npy') for n in ('tokens', 'encoded_lengths', 'log_probs')}
    assert all(a.dtype == np.float32 for a in got.values())

    dev = torch.device('cuda', 0)
    blob, _, fb, window, _, _ = bench.build_model(dev, 'QuartzNet15x5Base-En', 8, 8)
    fb, window = fb.to(dev), window.to(dev)
    S = line['config']['steps_in_flight']
    audio = torch.from_numpy(synth.make_audio(32, bench.SAMPLES, seed=100 + (steps - 1) % S)).to(dev)
    alen = torch.full((32,), bench.SAMPLES, dtype=torch.int32, device=dev)
    eng = engine.Engine(blob, 0, tile=128 if S > 1 else 32)
    logp, tokens, enc_len = eng.forward_audio(audio, alen, fb, window, engine.frontend_plan(fb), 0.97, 16, want_logp=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got['tokens'], tokens.cpu().numpy())
    np.testing.assert_array_equal(got['encoded_lengths'], enc_len.cpu().numpy())
    np.testing.assert_allclose(got['log_probs'], logp.cpu().numpy(), rtol=1e-6, atol=1e-6)
    eng.close()


def test_legacy_create_keeps_normalised_feats_and_read_tensor_refuses_unstored(golden_dir):
    """(a) An engine made through the rounds-1/2 entry qasr_engine_create keeps fuse_norm off: qasr_engine_forward_audio leaves
    the NORMALISED log-mel in `feats` (= qasr_frontend_mel, what the reference calls processed_signal, features.py:334-397),
    with the pad frames zero; a create_ex engine (fused normalisation) produces the same tokens.  (b) qasr_engine_read_tensor
    refuses tensors the launch plan never stores - a depthwise output inside the fused layer's launch, k_stem's
    intermediates - instead of returning stale arena bytes, and still serves the decoder's input."""
    from qasr import engine, melbank, pack
    from qasr.pack import OP_DW
    d = np.load(os.path.join(golden_dir, 'net_quartznet_w8a8.npz'))
    meta = json.loads(str(d['meta']))
    cfg = topology.quartznet15x5()
    blob, pm = pack.pack_model(cfg, synth.make_state_dict(cfg, meta['seed']), d['act_min'], d['act_max'], 8, 8)
    fb = torch.from_numpy(melbank.mel_filterbank(16000, 512, 64, 0.0, 8000.0).astype(np.float32)).cuda().contiguous()
    win = torch.hann_window(320, periodic=False).cuda()
    S = 40000
    audio = torch.from_numpy(synth.make_audio(3, S, seed=8)).cuda()
    alen = torch.tensor([S, S - 9001, 4000], dtype=torch.int32).cuda()
    plan = engine.frontend_plan(fb)
    want_feats, want_len = engine.frontend_mel(audio, alen, fb, win, 0.97, 16)
    e_old, e_new = engine.Engine(blob, 0, legacy_create=True), engine.Engine(blob, 0)
    feats = torch.full_like(want_feats, 7.0)                    # garbage a kernel must overwrite, pad frames included
    flen = torch.empty(3, dtype=torch.int32, device='cuda')
    _, tk_old, _ = e_old.forward_audio(audio, alen, fb, win, plan, 0.97, 16, feats=feats, feat_lens=flen)
    _, tk_new, _ = e_new.forward_audio(audio, alen, fb, win, plan, 0.97, 16)
    torch.cuda.synchronize()
    assert torch.equal(feats, want_feats) and torch.equal(flen, want_len)
    assert torch.equal(tk_old, tk_new)
    kinds, tens = pm['kinds'], pm['tensors']
    fused_dw_out = next(i for i, t in enumerate(tens) if t['producer'] >= 3 and kinds[t['producer']] == OP_DW)
    for tensor in (1, 2, fused_dw_out):                          # QUANT_IN output, block 0's depthwise output (k_stem), a fused dw output
        with pytest.raises(engine.QasrError, match='never materialised'):
            e_new.read_tensor(tensor, tens[tensor]['channels'])
    assert e_new.read_tensor(pm['dec_in'], 1024).shape[1] == 1024
    e_old.close()
    e_new.close()


def test_transcribe_runs_on_the_engine(tmp_path):
    """EncDecCTCModel.transcribe (ctc_models.py:148-212) of a calibrated model on the GPU: the forward passes go through the HIP
    engine (front-end with pad_to 0 + integer encoder / decoder), transcripts come back in input order and equal what the
    calibrated host modules decode from the same trimmed, padded batches through the same front-end features."""
    from nemo.collections.asr.data.audio_to_text import AudioToCharDataset, read_wav, trim_silence
    from nemo.collections.asr.metrics.wer import WER
    m = _prepared_model('QuartzNet15x5Base-En', seed=5, percentile=99.996, feat=64, frames=128)
    audio = synth.make_audio(3, 30000, seed=9)
    paths = []
    for i, n in enumerate((30000, 17000, 23456)):
        a = audio[i, :n].copy()
        a[:2000] = 0                                             # leading silence: trimmed away by the loader
        p = str(tmp_path / f'x{i}.wav')
        _write_wav(p, a)
        paths.append(p)
    hyps = m.transcribe(paths, batch_size=2)
    assert type(m._engine).__name__ == 'Engine' and len(hyps) == 3
    f = m.preprocessor.featurizer
    assert f.pad_to == 16 and f.dither > 0                       # restored
    f.dither, f.pad_to = 0.0, 0
    wer = WER(vocabulary=m.decoder.vocabulary)
    want = []
    for group in (paths[:2], paths[2:]):
        xs = [torch.from_numpy(np.ascontiguousarray(trim_silence(read_wav(p)))) for p in group]
        assert all(x.numel() < 30000 - 1000 for x in xs[:1])     # the silent head is gone
        sig = torch.zeros(len(xs), max(x.numel() for x in xs))
        for i, x in enumerate(xs):
            sig[i, :x.numel()] = x
        n = torch.tensor([x.numel() for x in xs])
        feats, flen = m._frontend_hip(sig.cuda(), n.cuda())
        e, _, sf = m.encoder(audio_signal=feats, length=flen)
        want += wer.ctc_decoder_predictions_tensor(m.decoder(encoder_output=e, encoder_output_scaling_factor=sf).argmax(-1))
    assert hyps == want
