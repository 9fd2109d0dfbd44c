"""The stacked FastGRNN classifier around the recurrent cell, mirroring the reference's
``RNNClassifierModel`` for ``rnn_name == "FastGRNNCUDA"`` (/root/reference model.py:22-233) as far as the hot
path goes: 1-3 ``FastGRNNCUDA`` layers, layer l's ``[T,B,H_l]`` output handed to layer l+1 (model.py:196-203),
``hidden2keyword = nn.Linear`` on the LAST state of the top layer (model.py:226-227), ``log_softmax``
(model.py:229-230), hidden-state carry between batches (``init_hidden`` / ``hidden_states``, model.py:150-156,
200-201) and the IHT hooks (model.py:91-107), all on the GPU.

Same constructor arguments, attribute and parameter names as the reference (``rnn_list.{l}.W|U|...``,
``hidden2keyword.weight|bias``: a reference state dict loads), with these differences:

* the top layer is asked for its last state only (``FastGRNNCUDA.forward(..., last_state=True)``): its backward
  then takes the ``[B,H]`` gradient directly instead of a dense ``[T,B,H]`` tensor that is zero except for one row,
  and under ``torch.no_grad()`` its hidden-state sequence is never written;
* ``loss(input, labels)`` computes ``nn.NLLLoss()(forward(input), labels)`` (trainClassifier.py:154,236) with the
  fused head kernel -- Linear, log_softmax, NLL and all their gradients in two launches;
* ``sparsify`` / ``sparsifyWithSupport`` work in place on the device (the reference moves every layer to the CPU
  and back, model.py:91-107);
* ``rnn_name="FastGRNNBatchNorm"`` builds ``kws_amd.FastGRNNBatchNorm`` layers (the reference's trained keyword
  spotter, model_batchnorm/): eval mode only (``model.eval()``; ``train()`` / ``eval()`` reach the layers as
  model.py:167-183 does), dense weights only, ``loss()`` stays a ``FastGRNNCUDA`` method.  The head reads the last
  time step of every utterance in both layouts; the reference's batch_first path indexes ``model_output[-1, :, :]``
  (model.py:225-227), i.e. the LAST UTTERANCE's state sequence, for a ``[B,T,H]`` output -- that is not reproduced;
* ``rnn_name="FastGRNNBatchNormCUDA"`` builds ``kws_amd.FastGRNNBatchNormCUDA`` layers: the same model trained on the
  GPU (training-mode BatchNorm; ``model.train()`` / ``model.eval()`` pick the mode as for ``"FastGRNNBatchNorm"``),
  and ``loss()`` trains it through the fused head;
* ``predict`` / ``batch_accuracy`` / ``evaluate`` (trainClassifier.py:54-65, 286-316) and ``detect_stream``
  (inferencetry.py:213-227) end in the fused inference head and the majority vote: scores, argmax, the count of
  correct rows and the detector's vote stay on the device;
* ``fit_audio`` is the loop of ``fit`` (trainClassifier.py:174-272) from an audio bank on the device, its batches,
  learning rates and IHT phases computed there by a ``kws_amd.TrainSchedule``: one captured graph replayed for the
  whole run, ``evaluate()`` after every epoch.  On a schedule built with ``rolling=True`` it is the reference's rolling
  mode: short early epochs, and every batch starting from the hidden-state bags of ``kws_amd.RollingBags``
  (model.py:135-156) instead of the zero state, the bag exchange captured with the rest.  Unlike the reference's,
  ``evaluate()`` there does not leak its last batch's states into the next training batch;
* the shadow ``rnn_list_`` / ``tracking`` ONNX-export path (model.py:72-84,187-195) is not built (export is
  disabled in the reference, trainClassifier.py:42-52).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .batchnorm import FastGRNNBatchNorm
from .batchnorm_train import FastGRNNBatchNormCUDA
from .head import head_predict, keyword_loss, vote_windows
from .fastgrnn_cuda import check_starts_range
from .graph import GraphedStep
from .optim import _FusedOptimizer
from .rnn import FastGRNNCUDA, gather_windows
from .rolling import RollingBags

_RNN_CLASSES = {"FastGRNNCUDA": FastGRNNCUDA, "FastGRNNBatchNorm": FastGRNNBatchNorm,     # model.py:12-15
                "FastGRNNBatchNormCUDA": FastGRNNBatchNormCUDA}


class RNNClassifierModel(nn.Module):
    """1-, 2- or 3-layer FastGRNN classifier (model.py:22-233), ``rnn_name`` ``"FastGRNNCUDA"`` or
    ``"FastGRNNBatchNorm"`` (eval mode)."""

    def __init__(self, rnn_name, input_dim, num_layers, hidden_units_list, wRank_list, uRank_list,
                 wSparsity_list, uSparsity_list, gate_nonlinearity, update_nonlinearity, num_classes=None,
                 linear=True, batch_first=False, apply_softmax=True, device=None):
        if rnn_name not in _RNN_CLASSES:
            raise ValueError("kws_amd builds the FastGRNNCUDA, FastGRNNBatchNorm and FastGRNNBatchNormCUDA model "
                             "families only (got %r)" % (rnn_name,))
        if linear and not num_classes:
            raise Exception("num_classes need to be specified if linear is True")      # model.py:54-56
        super().__init__()
        self.rnn_name = rnn_name
        self.input_dim = input_dim
        self.hidden_units_list = list(hidden_units_list)
        self.num_layers = num_layers
        self.num_classes = num_classes
        self.wRank_list, self.uRank_list = list(wRank_list), list(uRank_list)
        self.wSparsity_list, self.uSparsity_list = list(wSparsity_list), list(uSparsity_list)
        self.gate_nonlinearity = gate_nonlinearity
        self.update_nonlinearity = update_nonlinearity
        self.linear = linear
        self.batch_first = batch_first
        self.apply_softmax = apply_softmax
        self.rnn_list = nn.ModuleList([                                                 # model.py:61-70
            _RNN_CLASSES[rnn_name](self.input_dim if l == 0 else self.hidden_units_list[l - 1], self.hidden_units_list[l],
                         gate_nonlinearity=gate_nonlinearity, update_nonlinearity=update_nonlinearity,
                         wRank=self.wRank_list[l], uRank=self.uRank_list[l],
                         wSparsity=self.wSparsity_list[l], uSparsity=self.uSparsity_list[l],
                         batch_first=batch_first, device=device)
            for l in range(num_layers)])
        if self.linear:                                                                 # model.py:85-88
            self.hidden2keyword = nn.Linear(self.hidden_units_list[num_layers - 1], num_classes,
                                            device=self.rnn_list[0].device)
        self._batchnorm = rnn_name in ("FastGRNNBatchNorm", "FastGRNNBatchNormCUDA")
        self.init_hidden()

    # ---- bookkeeping (model.py:91-156) -----------------------------------------------------------------
    def sparsify(self):
        for rnn in self.rnn_list:
            rnn.sparsify()

    def sparsifyWithSupport(self):
        for rnn in self.rnn_list:
            rnn.sparsifyWithSupport()

    def get_model_size(self):
        total_size = 4 * self.hidden_units_list[self.num_layers - 1] * self.num_classes
        for rnn in self.rnn_list:
            total_size += rnn.get_model_size()
        return total_size

    def name(self):
        return f"{self.num_layers} layer {self.rnn_name}"

    def init_hidden(self):
        """Clear the carried hidden states (model.py:150-156)."""
        self.hidden_states = [None] * self.num_layers

    # ---- the hot path ------------------------------------------------------------------------------------
    def _last_state(self, input, windows=None):
        """Layers chained as model.py:196-203 does; returns the top layer's final state [B, H_top].  ``windows``:
        ``(pool, starts, T)`` -- layer 0 reads the batch as windows of a frame pool (``unroll_windows``; ``input`` is
        not used then)."""
        rnn_in = input
        top = self.num_layers - 1
        for l, rnn in enumerate(self.rnn_list):
            if self._batchnorm:                          # (model.py:211-215: the layers take the model's mode)
                out = rnn(rnn_in, hiddenState=self.hidden_states[l], training=self.training, last_state=(l == top))
            elif l == 0 and windows is not None:
                out = rnn.unroll_windows(*windows, hiddenState=self.hidden_states[0], last_state=(top == 0), check=False)
            else:
                out = rnn(rnn_in, hiddenState=self.hidden_states[l], last_state=(l == top))
            # (bf16 sequences: the state a layer carries over is fp32, like the one it starts from)
            if l == top:
                self.hidden_states[l] = out.detach().float()
            else:
                self.hidden_states[l] = (out.detach()[:, -1, :] if self.batch_first else out.detach()[-1, :, :]).float()
            rnn_in = out
        return rnn_in.float()                              # (the head is fp32; a no-op for fp32 sequences)

    def forward(self, input):
        """[T,B,F] (or [B,T,F] with ``batch_first``) -> keyword scores [B,C] (model.py:185-231)."""
        model_output = self._last_state(input)
        if self.linear:
            model_output = self.hidden2keyword(model_output)
        if self.apply_softmax:
            model_output = F.log_softmax(model_output, dim=1)
        return model_output

    def _window_states(self, stream, hop, window):
        """The layer chain of ``score_stream`` / ``detect_stream``: ``stream`` -> ``(h, S, Nw)``, ``h:[S*Nw,H_top]`` the
        top layer's last state of every window, each from a zero state."""
        if stream.dim() == 2:
            stream = stream[None]
        if stream.dim() != 3:
            raise ValueError("stream must be [streams, frames, features] or [frames, features]")
        S, L, Fn = stream.shape
        hop, window = int(hop), int(window)
        if hop < 1 or window < 1:
            raise ValueError("hop and window must be positive (got hop=%d, window=%d)" % (hop, window))
        if L < window:
            raise ValueError("stream of %d frames is shorter than the window of %d" % (L, window))
        dev = self.rnn_list[0].device
        pool = stream.to(dev).reshape(S * L, Fn)
        nw = (L - window) // hop + 1
        starts = (torch.arange(S, device=dev)[:, None] * L + torch.arange(nw, device=dev)[None, :] * hop).reshape(-1)
        top = self.num_layers - 1
        kw = {"training": self.training} if self._batchnorm else {}
        out = self.rnn_list[0].forward_windows(pool, starts, window, last_state=(top == 0), check=False, **kw)
        for l in range(1, self.num_layers):
            out = self.rnn_list[l](out, hiddenState=None, last_state=(l == top), **kw)
        return out, S, nw

    @torch.no_grad()
    def score_stream(self, stream, hop=1, window=99):
        """Score every window of continuous audio, as the reference's detector does one window at a time
        (inferencetry.py:165-227: a 99-frame window slid over the stream, the model run from a zero state on each).
        ``stream``: ``[S,L,F]`` (or ``[L,F]``: one stream) -> ``[S,Nw,C]`` scores, ``Nw = (L - window) // hop + 1``,
        window ``w`` of stream ``s`` being frames ``w*hop .. w*hop + window - 1``.  Layer 0 reads the stream in place
        (``forward_windows``: the window is the batch dimension, no ``window/hop``-fold copy); the layers above and
        the head run as ``forward`` does under ``torch.no_grad()``.  Every window starts from a zero state:
        ``hidden_states`` is neither read nor written.  ``detect_stream`` adds the argmax and the detector's majority
        vote over consecutive windows on the device.  BatchNorm models: eval mode only."""
        out, S, nw = self._window_states(stream, hop, window)
        out = out.float()
        if self.linear:
            out = self.hidden2keyword(out)
        if self.apply_softmax:
            out = F.log_softmax(out, dim=1)
        return out.reshape(S, nw, -1)

    @torch.no_grad()
    def detect_stream(self, stream, hop=1, window=99, num_windows=10, majority=5):
        """The reference's detector over continuous audio (inferencetry.py:165-227) without leaving the device:
        ``score_stream``'s chain with the fused inference head and the majority vote as its tail.  Returns
        ``(pred, majority, event)``, each ``[S,Nw]`` int32 on the device: ``pred`` the argmax of every window's scores
        (inferencetry.py:213-214), ``majority`` the most common of the last ``num_windows`` predictions where it has
        at least ``majority`` votes, else -1, and ``event`` that keyword at the windows where the reference prints
        "Detected keyword" (it differs from the last one reported, inferencetry.py:224-227), else -1.  Read detections
        out with ``event >= 0``: ``s, w = (event >= 0).nonzero(as_tuple=True)``, keyword ``event[s, w]``, window ``w``
        starting at frame ``w * hop``.  Streams vote independently, each from an empty list.  Needs ``linear=True``;
        BatchNorm models: eval mode only."""
        if not self.linear:
            raise RuntimeError("detect_stream() needs the Linear head (linear=True)")
        h, S, nw = self._window_states(stream, hop, window)
        pred, _, _ = head_predict(h.float().contiguous(), self.hidden2keyword.weight.contiguous(),
                                  self.hidden2keyword.bias.contiguous(), want_log_probs=False)
        pred = pred.reshape(S, nw)
        maj, event = vote_windows(pred, num_windows, majority)
        return pred, maj, event

    @torch.no_grad()
    def detect_audio(self, recording, frontend, hop_samples=800, num_windows=10, majority=5, clip=16000,
                     shared_frames=False):
        """The reference's live loop (inferencetry.py:165-227) end to end on raw audio: every ``hop_samples`` (50 ms)
        the last ``clip`` samples of the 1-D ``recording`` (fp32 or int16 PCM) are peak-normalised and featurised by
        ``frontend`` (a ``kws_amd.MFCCFrontend``; its ``mean`` / ``std`` and ``max_len`` are the model's), the model
        runs each clip from a zero state, and the majority vote runs over consecutive clips.  The clips are a strided
        view of the recording (``MFCCFrontend.clips_of``) and layer 0 reads the feature pool in place where the
        windowed scans hold the cell (``forward_windows`` with ``starts = arange(B) * max_len``; gathered elsewhere),
        so nothing is copied between the samples and the vote.  Returns what ``detect_stream`` returns for one stream:
        ``(pred, majority, event)``, each ``[1, B]`` int32 on the device, ``B = (N - clip) // hop_samples + 1``.
        ``hidden_states`` is neither read nor written.  Needs ``linear=True``; BatchNorm models: eval mode only.
        ``shared_frames=True`` featurises through ``frontend.stream``: every 10 ms frame of the recording goes through
        the DFT and the mel projection once instead of once per clip that contains it (features equal up to the fp32
        roundings of the peak scaling; everything behind the pool is unchanged).  It needs ``hop_samples`` a multiple
        of 160 and ``clip == 16000`` and raises ``ValueError`` otherwise: it never falls back to the per-clip path."""
        if not self.linear:
            raise RuntimeError("detect_audio() needs the Linear head (linear=True)")
        if frontend.num_features != self.input_dim:
            raise ValueError("the front end gives %d features, the model takes %d" % (frontend.num_features, self.input_dim))
        recording = recording.to(self.rnn_list[0].device)
        clips = None if shared_frames else frontend.clips_of(recording, hop_samples, clip)
        peak, frontend.peak_normalize = frontend.peak_normalize, True        # inferencetry.py:172-175
        try:                                                                 # [B, max_len, F]: the frame pool
            feats = frontend.stream(recording, hop_samples, clip) if shared_frames else frontend(clips)
        finally:
            frontend.peak_normalize = peak
        h, B, _ = self._window_states(feats, 1, feats.shape[1])              # (one window per clip: starts = b * max_len)
        pred, _, _ = head_predict(h.float().contiguous(), self.hidden2keyword.weight.contiguous(),
                                  self.hidden2keyword.bias.contiguous(), want_log_probs=False)
        pred = pred.reshape(1, B)
        maj, event = vote_windows(pred, num_windows, majority)
        return pred, maj, event

    def _predict(self, input, labels=None, want_log_probs=True):
        if not self.linear:
            raise RuntimeError("predict() / batch_accuracy() / evaluate() need the Linear head (linear=True)")
        h_last = self._last_state(input)
        if labels is not None:
            labels = labels.to(device=h_last.device, dtype=torch.int64).contiguous()
        return head_predict(h_last.contiguous(), self.hidden2keyword.weight.contiguous(),
                            self.hidden2keyword.bias.contiguous(), labels, want_log_probs)

    @torch.no_grad()
    def predict(self, input):
        """``(pred, log_probs)``: ``forward``'s keyword scores ``[B,C]`` (log-probabilities, model.py:226-230) and
        their argmax ``[B]`` int32, from the fused inference head.  Same layer chain and ``hidden_states`` carry as
        ``forward``, under ``torch.no_grad()``.  Needs ``linear=True``.  ``log_probs`` are log-probabilities whatever
        ``apply_softmax`` says: on a model built with ``apply_softmax=False``, whose ``forward`` returns the raw
        logits, they are ``log_softmax`` of those (the argmax is the same)."""
        pred, logp, _ = self._predict(input)
        return pred, logp

    @torch.no_grad()
    def batch_accuracy(self, input, labels):
        """The reference's ``batch_accuracy`` (trainClassifier.py:54-65) from the batch itself: runs ``predict`` on
        ``input`` and returns ``(percent, passed, results)`` -- ``results`` the predicted class of every utterance,
        ``passed`` how many equal ``labels``.  The reference compares row by row on the host (one sync per
        utterance); here the comparison and the count happen in the head kernel and one device-to-host copy at the
        end fetches both."""
        pred, _, n_correct = self._predict(input, labels, want_log_probs=False)
        host = torch.cat((n_correct, pred)).cpu().tolist()
        passed, results = host[0], host[1:]
        return (float(passed) * 100.0 / float(len(results)), passed, results)

    @torch.no_grad()
    def evaluate(self, batches):
        """The reference's ``evaluate`` (trainClassifier.py:286-316) over an iterable of ``(input, labels)``, ``input``
        in the layout ``forward`` takes: eval mode, ``init_hidden()`` before every batch (trainClassifier.py:304), the
        correct predictions counted by the head kernel and added up on the device; one sync, at the end.  Returns
        ``passed / total``."""
        self.eval()                                                     # trainClassifier.py:290
        passed, total = None, 0
        for input, labels in batches:
            self.init_hidden()
            _, _, n_correct = self._predict(input, labels, want_log_probs=False)
            passed = n_correct.to(torch.int64) if passed is None else passed + n_correct
            total += labels.numel()
        if total == 0:
            raise ValueError("evaluate: no batches")
        return int(passed) / total

    def loss(self, input, labels):
        """``nn.NLLLoss()(self(input), labels)`` (trainClassifier.py:233-236) with the fused head."""
        if self.rnn_name == "FastGRNNBatchNorm":
            raise NotImplementedError("loss() trains FastGRNNCUDA models; FastGRNNBatchNorm runs in eval mode only")
        if not (self.linear and self.apply_softmax):
            raise RuntimeError("loss() is the Linear + log_softmax + NLLLoss tail (linear=True, apply_softmax=True)")
        h_last = self._last_state(input)
        return keyword_loss(h_last, self.hidden2keyword.weight, self.hidden2keyword.bias, labels)

    def train_step(self, input, labels, optimizer, iht="none", bucket=None):
        """One trainer iteration (trainClassifier.py:230-259) on the device: gradients set to None, ``loss()``,
        ``backward()``, the gradient all-reduce of ``bucket`` (a ``kws_amd.dp.GradBucket``) if given, then
        ``optimizer.step(iht)``.  ``optimizer`` must be a ``kws_amd.FusedAdam`` / ``FusedSGD`` (``TypeError`` otherwise:
        a torch optimizer's ``step()`` has no IHT phase): the update of every parameter and the IHT
        phase ``iht`` (``"none"``, ``"threshold"``, ``"support"``: what ``kws_amd.iht_phase`` returns for the
        iteration, or ``None`` to leave the optimizer's ``iht_t`` as it is) in one library call.  Returns the detached
        loss.  Nothing here synchronises, so the whole step captures in a ``GraphedStep`` (build the optimizer with
        ``capturable=True`` and write its ``lr_t`` / ``iht_t`` between replays).

        The fused optimizer owns the support masks of its IHT phases (``optimizer.support(param)``); it neither reads
        nor writes a layer's ``oldmats``, and ``sparsify()`` / ``sparsifyWithSupport()`` stay as they are.  The two
        mechanisms are not meant to be mixed within one run."""
        if not isinstance(optimizer, _FusedOptimizer):
            raise TypeError("train_step() needs a kws_amd.FusedAdam or kws_amd.FusedSGD, or another fused optimizer of "
                            "kws_amd.optim (got %s): a torch optimizer's "
                            "step() has no IHT phase -- call loss(), backward(), optimizer.step() and sparsify() yourself"
                            % type(optimizer).__name__)
        for p in self.parameters():
            p.grad = None
        loss = self.loss(input, labels)
        loss.backward()
        if bucket is not None:
            bucket.all_reduce_()
        optimizer.step(iht)
        return loss.detach()

    def train_step_audio(self, audio, lengths, labels, index, frontend, augment, optimizer, iht="none", bucket=None,
                         check=False):
        """``train_step`` from raw audio that lives on the device: ``audio:[N,L]`` is the dataset as an audio bank
        (float32 samples or int16 PCM), ``lengths:[N]`` int32 or None, ``labels:[N]``; the batch is ``index:[B]`` int32
        clip indices, freshly augmented.  ``records = augment.draw(index, optimizer.step_t)`` (a ``kws_amd.AudioAugment``;
        the step scalar is read as it stands BEFORE this step's update), the features come from ``frontend`` (a
        ``kws_amd.MFCCFrontend``) reading the bank through the records under ``torch.no_grad()`` -- no augmented audio
        and no gathered batch is written --, ``labels[index]`` is gathered on the device, and the rest is exactly
        ``train_step`` on those features: layer 0 reads the ``[B, max_len, F]`` feature pool in place where
        ``loss_windows`` can (``starts = arange(B) * max_len``), ``hidden_states`` is carried as there.  Returns the
        detached loss.  Nothing synchronises with ``check=False`` (``check=True`` validates ``index`` and the records on
        the host first), so the step captures in a ``GraphedStep``: ``index`` is a captured input that the caller
        overwrites between replays, and every replay draws new augmentations as ``step_t`` advances."""
        if not isinstance(optimizer, _FusedOptimizer):
            raise TypeError("train_step_audio() needs a kws_amd.FusedAdam or kws_amd.FusedSGD, or another fused "
                            "optimizer of kws_amd.optim (got %s)"
                            % type(optimizer).__name__)
        if self.rnn_name == "FastGRNNBatchNorm":
            raise NotImplementedError("loss() trains FastGRNNCUDA models; FastGRNNBatchNorm runs in eval mode only")
        if not (self.linear and self.apply_softmax):
            raise RuntimeError("loss() is the Linear + log_softmax + NLLLoss tail (linear=True, apply_softmax=True)")
        if frontend.num_features != self.input_dim:
            raise ValueError("the front end gives %d features, the model takes %d" % (frontend.num_features, self.input_dim))
        records = augment.draw(index, optimizer.step_t)
        with torch.no_grad():
            feats = frontend(audio, lengths, augment=records, noise=augment.noise, noise_lengths=augment.noise_lengths,
                             check=check)                                    # [B, max_len, F]: the frame pool
            target = labels.index_select(0, index)
        for p in self.parameters():
            p.grad = None
        B, T, Fn = feats.shape
        if self._batchnorm:
            h_last = self._last_state(feats if self.batch_first else feats.transpose(0, 1).contiguous())
        else:
            key = (B, T, feats.device)
            if getattr(self, "_audio_starts", (None,))[0] != key:            # (built once per batch shape)
                self._audio_starts = (key, torch.arange(B, device=feats.device, dtype=torch.int32) * T)
            h_last = self._last_state(None, windows=(feats.view(B * T, Fn), self._audio_starts[1], T))
        loss = keyword_loss(h_last, self.hidden2keyword.weight, self.hidden2keyword.bias, target)
        loss.backward()
        if bucket is not None:
            bucket.all_reduce_()
        optimizer.step(iht)
        return loss.detach()

    def fit_audio(self, audio, lengths, labels, frontend, augment, optimizer, schedule, *, graph=True, bucket=None,
                  validation=None, bags=None):
        """A whole training run (trainClassifier.py:174-272) from the audio bank, driven by a
        ``kws_amd.TrainSchedule``: ``schedule.total_iterations`` (``num_epochs * ticks``) iterations of

            init_hidden()                    (trainClassifier.py:221: every batch starts from the zero state)
            schedule.advance()               index, lr_t, iht_t and the position from optimizer.step_t
            loss = train_step_audio(audio, lengths, labels, schedule.index, frontend, augment, optimizer, iht=None)
            schedule.record(loss)

        On a schedule built with ``rolling=True`` (the reference's ``--rolling``) the body is instead

            schedule.advance()               ... at the rolling position: short early epochs
            bags.exchange()                  the last states into the hidden bags, this batch's start out of them
            loss = train_step_audio(...)
            bags.commit()                    this batch's last states, for the next exchange
            schedule.record(loss)

        with ``bags`` a ``kws_amd.RollingBags(self, schedule)``, built here unless the caller passes its own to look
        into.  The carried states live in ``bags``, so the validation passes between epochs cannot disturb them.

        With ``graph=True`` that body is captured once in a ``GraphedStep`` and replayed; nothing is written from the
        host between replays, and the run starts from the state the model and the optimizer were in: the capture's
        warm-up iterations are undone by ``GraphedStep(body, undo=[self, optimizer, schedule, bags])``, each of the four
        listing in its ``run_tensors()`` what an iteration carries over to the next (parameters and buffers; ``step_t``,
        support masks, guard state and the rule's state; the logs; the bags).  ``lr_t`` and ``iht_t`` are in no list,
        ``advance()`` rewrites both every iteration; optimizer state that the warm-up created goes back to what the rule
        creates it with (``run_reset``).
        ``graph=False`` runs the same body eagerly and gives the same bits.  The run begins at ``optimizer.step_t`` as it
        stands (0 for a fresh optimizer; one sync, before the first iteration) and ends at iteration
        ``num_epochs * ticks`` counted from 0.
        ``validation``: an iterable of ``(input, labels)`` batches, or a callable returning one, handed to ``evaluate()``
        after every epoch -- the only sync inside the run; the model is put back in training mode afterwards.  Returns
        the reference's log: one ``{"epoch", "loss", "accuracy", "learning_rate"}`` per epoch, the epoch's last loss and
        learning rate read from ``schedule.loss_log`` / ``lr_log`` at the end."""
        if not isinstance(optimizer, _FusedOptimizer):
            raise TypeError("fit_audio() needs a kws_amd.FusedAdam or kws_amd.FusedSGD, or another fused optimizer of "
                            "kws_amd.optim (got %s)" % type(optimizer).__name__)
        if getattr(schedule, "optimizer", None) is not optimizer:
            raise ValueError("fit_audio(): the schedule was built for another optimizer (it writes that one's lr_t / iht_t)")
        if labels.shape[0] != schedule.num_clips or audio.shape[0] != schedule.num_clips:
            raise ValueError("fit_audio(): the schedule shuffles %d clips, the bank holds %d with %d labels"
                             % (schedule.num_clips, audio.shape[0], labels.shape[0]))

        rolling = bool(getattr(schedule, "rolling", False))
        if rolling and bags is None:
            bags = RollingBags(self, schedule)
        if bags is not None and (not rolling or bags.schedule is not schedule or bags.model is not self):
            raise ValueError("fit_audio(): bags go with a rolling schedule, and must have been built for this model and "
                             "this schedule")

        def body():
            if rolling:
                schedule.advance()
                bags.exchange()
            else:
                self.init_hidden()
                schedule.advance()
            loss = self.train_step_audio(audio, lengths, labels, schedule.index, frontend, augment, optimizer, iht=None,
                                         bucket=bucket)
            if rolling:
                bags.commit()
            schedule.record(loss)
            return loss

        self.train()
        step = body
        if graph:
            step = GraphedStep(body, undo=[self, optimizer, schedule] + ([bags] if bags is not None else []))
        first = int(optimizer.step_t.item())
        accuracies = [None] * schedule.num_epochs
        for s in range(first, schedule.total_iterations):
            step()
            if validation is not None and schedule.epoch_end(s):
                accuracies[schedule.position(s)[0]] = self.evaluate(validation() if callable(validation) else validation)
                self.train()
        return schedule.epoch_log(accuracies)

    def run_tensors(self):
        """What a training step carries over to the next here (``kws_amd.graph.RunSnapshot``): parameters and buffers."""
        return list(self.parameters()) + list(self.buffers())

    def run_reset(self, held_ids):
        self.init_hidden()                                    # (the carried states are results, not tensors kept here)

    def loss_windows(self, pool, starts, labels, window=99):
        """``loss()`` on the batch whose utterance ``b`` is the ``window`` consecutive rows of ``pool:[R,F]`` from row
        ``starts[b]`` on -- a training step from a frame pool that lives on the device: the batch is ``B`` start rows
        (random time-shift crops are other start rows), with no host batch assembly and no ``[B,T,F]`` tensor kept for
        the backward.  Layer 0 goes through ``FastGRNNCUDA.unroll_windows``; the layers above and the fused head run
        as in ``loss()``, and ``hidden_states`` is carried exactly as there.  The starts' range is checked once here
        (``ValueError``).  BatchNorm model families gather the windows in front of layer 0: training-mode BatchNorm
        over windows is not built."""
        if self.rnn_name == "FastGRNNBatchNorm":
            raise NotImplementedError("loss() trains FastGRNNCUDA models; FastGRNNBatchNorm runs in eval mode only")
        if not (self.linear and self.apply_softmax):
            raise RuntimeError("loss() is the Linear + log_softmax + NLLLoss tail (linear=True, apply_softmax=True)")
        window = int(window)
        if self._batchnorm:
            h_last = self._last_state(gather_windows(pool.to(self.rnn_list[0].device), starts.to(self.rnn_list[0].device),
                                                     window, batch_first=self.batch_first))
        else:
            if pool.requires_grad:
                raise ValueError("loss_windows: the pool must not require grad (unroll_windows)")
            dev = self.rnn_list[0].device
            pool, starts = pool.to(dev), starts.to(dev)
            check_starts_range(starts, pool.shape[0], window)
            h_last = self._last_state(None, windows=(pool, starts, window))
        return keyword_loss(h_last, self.hidden2keyword.weight, self.hidden2keyword.bias, labels)
