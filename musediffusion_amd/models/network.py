"""TransformerNetModel: the denoiser behind the reference's plugin surface, executed by libmusehip.

Drop-in for MuseDiffusion/models/network.py:20-158: same constructor arguments, same methods
(`get_embeds`, `get_logits`, `timestep_embedding`, `forward(x, timesteps, **_)`), same attributes
(`word_embedding`, `lm_head` tied to it, `time_embed`, `input_up_proj`, `input_transformers`,
`position_embeddings`, `LayerNorm`, `output_down_proj`) and therefore the same `state_dict()` keys —
checkpoints written by the reference load unchanged.

What differs is where the arithmetic runs: parameters stay ordinary fp32 `nn.Parameter`s (so
optimizers / DDP / EMA / checkpoint code keep working), but `forward` packs them into a device
weight arena (engine.DenoiserEngine, re-packed only when a parameter changes) and runs the whole
network as one `mh_denoiser_forward` call of hand-written gfx950 kernels.  CPU tensors are refused:
there is no fallback path.

The reference hard-codes the Transformer shape to bert-base-uncased (network.py:44-46).  Here the
shape is a keyword-only constructor argument defaulting to those values, so the BASELINE configs
(2-layer d=128, 12-layer d=512) are reachable without monkey-patching.
"""

import torch
import torch.nn as nn

from .. import _lib, ops
from ..engine import DenoiserEngine


# ---- parameter containers mirroring the HF BertEncoder module tree (names only; no HF code runs) ----
class _SelfAttention(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.query = nn.Linear(H, H)
        self.key = nn.Linear(H, H)
        self.value = nn.Linear(H, H)


class _DenseNorm(nn.Module):
    def __init__(self, fan_in, H, eps):
        super().__init__()
        self.dense = nn.Linear(fan_in, H)
        self.LayerNorm = nn.LayerNorm(H, eps=eps)


class _Attention(nn.Module):
    def __init__(self, H, eps):
        super().__init__()
        setattr(self, "self", _SelfAttention(H))
        self.output = _DenseNorm(H, H, eps)


class _Intermediate(nn.Module):
    def __init__(self, H, F):
        super().__init__()
        self.dense = nn.Linear(H, F)


class _Layer(nn.Module):
    def __init__(self, H, F, eps):
        super().__init__()
        self.attention = _Attention(H, eps)
        self.intermediate = _Intermediate(H, F)
        self.output = _DenseNorm(F, H, eps)


class _Encoder(nn.Module):
    """Holds `layer.{i}.…` parameters under the names HF's BertEncoder uses (network.py:74)."""

    def __init__(self, H, F, n_layers, eps):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(H, F, eps) for _ in range(n_layers)])


class TransformerNetModel(nn.Module):
    """
    The full Transformer denoiser with attention and timestep embedding (network.py:20-29).

    :param input_dims: dims of the input Tensor (latent width E).
    :param output_dims: dims of the output Tensor.
    :param hidden_t_dim: dims of time embedding.
    :param vocab_size: the size of vocabulary.
    :param seq_len: maximum sequence length (size of the learned position table).
    :param dropout: rate of the dropout after the embedding LayerNorm in train mode (network.py:76, :149).
    :param bert_hidden/bert_layers/bert_heads/bert_ffn: Transformer shape (default bert-base-uncased).
    :param bert_hidden_dropout/bert_attention_dropout: the encoder's own train-mode dropouts; the reference leaves them at
           bert-base's 0.1 / 0.1 whatever `dropout` is (network.py:44-46).  `model.eval()` turns all three off.
    :param compute_dtype: "fp32" (parity mode: fp32 storage + exact-fp32 MFMA) or "bf16"
                          (throughput mode: bf16 storage, bf16 MFMA, fp32 accumulation).
    """

    def __init__(self, input_dims, output_dims, hidden_t_dim, vocab_size, seq_len, dropout=0.1, logits_mode=1, *,
                 bert_hidden=768, bert_layers=12, bert_heads=12, bert_ffn=3072, layer_norm_eps=1e-12,
                 bert_hidden_dropout=0.1, bert_attention_dropout=0.1, compute_dtype="fp32"):
        super().__init__()
        if input_dims != output_dims:
            raise ValueError("input_dims and output_dims must match (the reference always passes hidden_dim twice, "
                             "utils/initialization.py:114-121)")
        if bert_hidden % bert_heads:
            raise ValueError("bert_heads must divide bert_hidden")
        self.input_dims = input_dims
        self.hidden_t_dim = hidden_t_dim
        self.output_dims = output_dims
        self.logits_mode = logits_mode
        self.hidden_size = bert_hidden
        self.num_heads = bert_heads
        self.ffn_size = bert_ffn
        self.seq_len = seq_len
        self.vocab_size = vocab_size
        self.compute_dtype = compute_dtype
        # the reference's BertEncoder keeps bert-base's dropouts (0.1 / 0.1) whatever `dropout` is (network.py:44-46, :74)
        self.bert_hidden_dropout = float(bert_hidden_dropout)
        self.bert_attention_dropout = float(bert_attention_dropout)
        self.dropout_masks = None          # tests: explicit keep masks per site (training._DropSites)
        self._dropout_seed = None
        self._dropout_calls = 0

        # construction order follows network.py:55-86 so that a seeded default init draws alike
        self.word_embedding = nn.Embedding(vocab_size, input_dims)
        self.lm_head = nn.Linear(input_dims, vocab_size)
        with torch.no_grad():
            self.lm_head.weight = self.word_embedding.weight
        time_embed_dim = hidden_t_dim * 4
        self.time_embed = nn.Sequential(nn.Linear(hidden_t_dim, time_embed_dim), nn.SiLU(),
                                        nn.Linear(time_embed_dim, bert_hidden))
        if input_dims != bert_hidden:
            self.input_up_proj = nn.Sequential(nn.Linear(input_dims, bert_hidden), nn.Tanh(),
                                               nn.Linear(bert_hidden, bert_hidden))
        self.input_transformers = _Encoder(bert_hidden, bert_ffn, bert_layers, layer_norm_eps)
        self.dropout = nn.Dropout(dropout)
        self.register_buffer("position_ids", torch.arange(seq_len).expand((1, -1)))
        self.position_embeddings = nn.Embedding(seq_len, bert_hidden)
        self.LayerNorm = nn.LayerNorm(bert_hidden, eps=layer_norm_eps)
        if output_dims != bert_hidden:
            self.output_down_proj = nn.Sequential(nn.Linear(bert_hidden, bert_hidden), nn.Tanh(),
                                                  nn.Linear(bert_hidden, output_dims))
        self._engine = None
        self._engine_key = None
        self._table_norm = None
        self.weights_from_arena = False

    # ------------------------------------------------------------------ engine management
    def pin_engine(self):
        """The engine's arena was filled from outside (one packed RCCL broadcast): keep it instead of re-packing from
        this rank's fp32 parameters, which no longer describe the weights."""
        self._engine_key = self._weights_key()
        self._table_norm = None
        self.weights_from_arena = True
        return self

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.weights_from_arena = False
        self._engine_key = None
        return out

    def _weights_key(self):
        ps = list(self.parameters())
        return (self.compute_dtype, str(ps[0].device)) + tuple((p.data_ptr(), p._version) for p in ps)

    def engine(self):
        """The packed-weight engine for the current parameter values (rebuilt when they change)."""
        dev = self.word_embedding.weight.device
        if dev.type != "cuda":
            raise _lib.MuseHipError("TransformerNetModel runs on the GPU only: call .to('cuda') first "
                                    "(no CPU fallback exists)")
        key = self._weights_key()
        if self.weights_from_arena:
            if self._engine_key != key:
                raise _lib.MuseHipError("this rank's engine holds broadcast weights (sharding.broadcast_weights(packed=True)) "
                                        "but its fp32 parameters changed: load a state_dict or broadcast flat parameters first")
            return self._engine
        if self._engine is None or self._engine_key != key:
            if self._engine is None or self._engine.device != dev or self._engine.dtype != ops.dtype_code(self.compute_dtype):
                cfg = dict(E=self.input_dims, H=self.hidden_size, F=self.ffn_size, nh=self.num_heads,
                           nL=len(self.input_transformers.layer), Tt=self.hidden_t_dim, L_max=self.seq_len,
                           ln_eps=self.LayerNorm.eps)
                self._engine = DenoiserEngine(cfg, self.compute_dtype, dev)
            self._engine.load_state_dict(dict(self.state_dict()))
            self._engine_key = key
            self._table_norm = None
        return self._engine

    def dropout_seed(self):
        """Philox key of this model's dropout masks: fixed at the first training forward from torch's seed (so `torch.manual_seed`
        makes runs repeatable) and mixed with the rank, so data-parallel replicas drop different units like the reference's
        per-process generators do."""
        if self._dropout_seed is None:
            import torch.distributed as dist
            r = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            self._dropout_seed = (int(torch.initial_seed()) * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * (r + 1)) & (2 ** 64 - 1)
        return self._dropout_seed

    def next_dropout_call(self):
        self._dropout_calls += 1
        return self._dropout_calls

    def set_compute_dtype(self, compute_dtype):
        ops.dtype_code(compute_dtype)
        self.compute_dtype = compute_dtype
        self._engine = None
        return self

    def embedding_norms(self):
        """|W_v|^2 per vocabulary row, cached with the engine (rounding.py:22)."""
        self.engine()
        if self._table_norm is None:
            self._table_norm = ops.row_sqnorm(self.word_embedding.weight.detach())
        return self._table_norm

    # ------------------------------------------------------------------ reference API
    def get_embeds(self, input_ids):
        """network.py:88-89."""
        w = self.word_embedding.weight
        _lib.require_device(w)
        return ops.embed_gather(w.detach(), input_ids.to(w.device))

    def get_logits(self, hidden_repr):
        """network.py:91-106: logits_mode 1 = lm_head(x) (the only mode the reference ever constructs); 2 = the negative Euclidean distance of
        every position to every lm_head row, -sqrt(clamp(|W_v|^2 + |x_n|^2 - 2 W_v.x_n, 0)) (network.py:94-104; lm_head.bias is not used)."""
        if self.logits_mode not in (1, 2):
            raise NotImplementedError
        w, b = self.lm_head.weight.detach(), self.lm_head.bias.detach()
        _lib.require_device(w, hidden_repr)
        V, E = w.shape
        Ep = ops.pad64(E)
        flat = hidden_repr.reshape(-1, E).to(torch.float32)
        x = ops.cast_pad(flat, Ep, _lib.MH_F32)
        wp = ops.cast_pad(w, Ep, _lib.MH_F32)
        out = ops.gemm_bias_act(x, wp, b if self.logits_mode == 1 else None, None, None, _lib.MH_F32, out_f32=True, N=V, K=Ep)
        if self.logits_mode == 2:
            wn, xn = ops.row_sqnorm(w), ops.row_sqnorm(flat)
            scores = torch.empty(flat.shape[0], V, device=flat.device, dtype=torch.float32)
            _lib.check(_lib.lib().mh_distance_scores(_lib.ptr(out), out.shape[1], _lib.ptr(wn), _lib.ptr(xn), _lib.ptr(scores), V, flat.shape[0], V,
                                                     _lib.current_stream()), "mh_distance_scores")
            return scores.view(*hidden_repr.shape[:-1], V)
        return out.view(*hidden_repr.shape[:-1], V)

    def argmax_tokens(self, hidden_repr, constrain=None):
        """argmax(get_logits(x), -1) without materialising the logits (run/sample.py:219-220), in the model's logits_mode.
        constrain (an addition): None, or (input_ids, input_mask[, bars]) of the rows - then the note region of every row is the best
        sequence the decode path accepts instead (utils/grammar_util.constrain_tokens) and the return is (tokens, ConstrainResult);
        or an infill plan (utils/infill_util.InfillPlan) - then the plan's masked slots hold whole notes instead
        (utils/grammar_util.constrain_region_tokens) and the return is (tokens, RegionResult)."""
        if self.logits_mode not in (1, 2):
            raise NotImplementedError
        if constrain is not None:
            from ..utils.grammar_util import constrain_region_tokens, constrain_tokens
            if isinstance(constrain, (tuple, list)):
                return constrain_tokens(self, hidden_repr, *constrain)
            return constrain_region_tokens(self, hidden_repr, constrain)
        w, b = self.lm_head.weight.detach(), self.lm_head.bias.detach()
        if self.logits_mode == 2:
            # |W_v|^2: the cache that follows the engine (refreshed with it when any parameter's version changes) while lm_head is tied
            # to the embedding; after overload_embedding (utils/initialization.py:61-63) lm_head has rows of its own
            tied = w.data_ptr() == self.word_embedding.weight.data_ptr()
            wn = self.embedding_norms() if tied else ops.row_sqnorm(w)
            idx = ops.distance_argmax(hidden_repr.to(torch.float32), w, wn)
        else:
            idx = ops.logits_argmax(hidden_repr.to(torch.float32), w, b)
        return idx.view(hidden_repr.shape[:-1]).long()

    @staticmethod
    def timestep_embedding(timesteps, dim, max_period=10000):
        """Sinusoidal timestep embeddings, fractional timesteps allowed (network.py:108-129)."""
        _lib.require_device(timesteps)
        return ops.timestep_embedding(timesteps.reshape(-1), dim, _lib.MH_F32, dim, max_period)

    def forward(self, x, timesteps, **_):
        """
        Apply the model to an input batch (network.py:131-158).

        :param x: an [N x L x C] Tensor of inputs.
        :param timesteps: a 1-D batch of (possibly fractional) timesteps.
        :return: an [N x L x C] Tensor of outputs.
        """
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if self.weights_from_arena:
                raise _lib.MuseHipError("cannot train on a rank whose weights arrived as a packed inference arena")
            from ..training import denoiser_forward_with_grad
            return denoiser_forward_with_grad(self, x, timesteps)
        eng = self.engine()
        _lib.require_device(x)
        emb_t = eng.time_embed(timesteps.to(x.device))
        return eng.forward(x, emb_t).type(x.dtype)
