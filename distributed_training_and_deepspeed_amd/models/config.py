"""Built-in model configurations (no hub access on the MI355X boxes).

The reference pulls configs/weights from the HF hub
(``data_parallel_training.py:30-31``, ``model_parallel_training.py:36``,
``zero_dp_training.py:24``).  There is no network here, so every architecture the
reference trains is described by a built-in preset with random initialisation.
Parameter counts are checked in ``tests/test_models_cpu.py`` against the values
derived in SURVEY.md section 6 (bert-base MLM 108,340,804; bloom-560m 559,214,592;
opt-125m 125,239,296; gpt2-medium 354,823,168).
"""
from __future__ import annotations

from dataclasses import asdict, dataclass, field, replace


@dataclass(frozen=True)
class TransformerConfig:
    name: str
    family: str  # "bert" | "bloom" | "opt" | "gpt2" | "llama" | "block"
    vocab_size: int
    hidden_size: int
    num_layers: int
    num_heads: int
    ffn_size: int
    max_positions: int = 512
    type_vocab_size: int = 0          # BERT token-type embeddings
    position_offset: int = 0          # OPT learned positions are offset by 2
    activation: str = "gelu"          # "gelu" (erf) | "gelu_tanh" | "relu" | "swiglu" (gated, see below)
    pre_ln: bool = False              # False = post-LN (BERT)
    causal: bool = False
    alibi: bool = False               # BLOOM ALiBi position bias
    embedding_ln: bool = False        # LN right after the embeddings (BERT, BLOOM)
    final_ln: bool = False            # final LN before the LM head (pre-LN models)
    mlm_head: bool = False            # BERT transform (dense+act+LN) + decoder bias
    tie_word_embeddings: bool = True
    ln_eps: float = 1e-5
    hidden_dropout: float = 0.1
    attn_dropout: float = 0.1
    bias: bool = True
    pad_token_id: int = 0
    special_token_ids: tuple = field(default_factory=tuple)
    mask_token_id: int = -1
    norm: str = "layer"               # "layer" (LayerNorm) | "rms" (RMSNorm: no mean, no beta)
    rope_theta: float = 0.0           # rotary position embedding base; 0 = off
    num_kv_heads: int = 0             # grouped-query attention (Llama family): key/value heads; 0 = num_heads
    sliding_window: int = 0           # causal sliding-window attention (Mistral): keys per query, own included; 0 = off
    num_experts: int = 0              # mixture-of-experts FFN (Mixtral, models/moe.py): experts per layer; 0 = dense
    experts_per_token: int = 2        # experts each token is routed to (top-k)
    moe_capacity_factor: float = 0.0  # slots per expert = cf * T * k / E, rounded up to 8 (DeepSpeed); 0.0 = dropless
    router_aux_loss_coef: float = 0.0  # weight of the load-balancing loss in the model's loss
    # activation "swiglu": the gated MLP down(silu(gate(x)) * up(x)), three weights, no bias

    def __post_init__(self):
        if self.norm not in ("layer", "rms"):
            raise ValueError(f"norm must be 'layer' or 'rms', got {self.norm!r}")
        if self.norm == "rms" and self.hidden_dropout > 0:
            raise ValueError("norm='rms' has no fused residual dropout: hidden_dropout must be 0")
        if self.rope_theta > 0 and self.alibi:
            raise ValueError("rope_theta > 0 and alibi are two position schemes: pick one")
        if self.rope_theta > 0 and self.head_dim not in (64, 128):
            raise ValueError(f"rotary embeddings need head_dim 64 or 128 (the flash attention kernels), "
                             f"got {self.head_dim}")
        if self.activation == "swiglu" and self.bias:
            raise ValueError("activation='swiglu' is the bias-free gated MLP: bias must be False")
        traits = (self.norm == "rms", self.rope_theta > 0, self.activation == "swiglu")
        if any(traits) and not (all(traits) and self.pre_ln and not self.bias):
            raise ValueError("norm='rms', rope_theta > 0 and activation='swiglu' come together, pre-LN and "
                             "bias-free (models/llama.py::LlamaLayer is the one layer that implements them)")

        if self.num_kv_heads < 0 or (self.num_kv_heads and self.num_heads % self.num_kv_heads):
            raise ValueError(f"num_kv_heads = {self.num_kv_heads} must divide num_heads = {self.num_heads}")
        if self.kv_heads != self.num_heads and not self.llama_style:
            raise ValueError("grouped-query attention (num_kv_heads != num_heads) is implemented by "
                             "models/llama.py::LlamaLayer only")
        if self.kv_heads != self.num_heads and self.attn_dropout > 0:
            raise ValueError("grouped-query attention has no attention dropout: attn_dropout must be 0")
        if self.sliding_window < 0:
            raise ValueError(f"sliding_window = {self.sliding_window} must be >= 0 (0 = off)")
        if self.sliding_window and not (self.llama_style and self.causal and self.attn_dropout == 0):
            raise ValueError("a sliding window (sliding_window > 0) is implemented by models/llama.py::LlamaLayer "
                             "only, for causal models without attention dropout")

        if self.num_experts < 0:
            raise ValueError(f"num_experts = {self.num_experts} must be >= 0 (0 = dense)")
        if self.num_experts and not self.llama_style:
            raise ValueError("a mixture-of-experts FFN (num_experts > 0) is implemented by models/moe.py::MoeLlamaLayer "
                             "only, for the Llama family")
        if self.num_experts and not 1 <= self.experts_per_token <= self.num_experts:
            raise ValueError(f"experts_per_token = {self.experts_per_token} must be in [1, num_experts = "
                             f"{self.num_experts}]")
        if self.moe_capacity_factor < 0:
            raise ValueError(f"moe_capacity_factor = {self.moe_capacity_factor} must be >= 0 (0 = dropless)")

    @property
    def kv_heads(self) -> int:
        """Key/value heads: ``num_kv_heads``, or ``num_heads`` when that is 0 (multi-head attention)."""
        return self.num_kv_heads or self.num_heads

    @property
    def llama_style(self) -> bool:
        return self.activation == "swiglu"

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    def with_(self, **kw) -> "TransformerConfig":
        return replace(self, **kw)

    def to_dict(self) -> dict:
        return asdict(self)


# bert-base-cased / bert-large-cased (HF BertConfig defaults; special ids PAD 0, UNK 100,
# CLS 101, SEP 102, MASK 103 of the cased vocab) -- SURVEY.md D15/D19.
_BERT_SPECIAL = (0, 100, 101, 102, 103)

BERT_BASE = TransformerConfig(
    name="bert-base-cased", family="bert", vocab_size=28996, hidden_size=768, num_layers=12,
    num_heads=12, ffn_size=3072, max_positions=512, type_vocab_size=2, activation="gelu",
    pre_ln=False, causal=False, embedding_ln=True, mlm_head=True, ln_eps=1e-12,
    hidden_dropout=0.1, attn_dropout=0.1, pad_token_id=0, special_token_ids=_BERT_SPECIAL,
    mask_token_id=103,
)
BERT_LARGE = BERT_BASE.with_(name="bert-large-cased", hidden_size=1024, num_layers=24,
                             num_heads=16, ffn_size=4096)
# Small config for CPU/gloo plumbing tests (BASELINE config 1).
BERT_TINY = BERT_BASE.with_(name="bert-tiny", vocab_size=1024, hidden_size=128, num_layers=2,
                            num_heads=2, ffn_size=512, max_positions=512)

BLOOM_560M = TransformerConfig(
    name="bigscience/bloom-560m", family="bloom", vocab_size=250880, hidden_size=1024,
    num_layers=24, num_heads=16, ffn_size=4096, max_positions=2048, activation="gelu_tanh",
    pre_ln=True, causal=True, alibi=True, embedding_ln=True, final_ln=True, ln_eps=1e-5,
    hidden_dropout=0.0, attn_dropout=0.0, pad_token_id=3, special_token_ids=(0, 1, 2, 3),
)
OPT_125M = TransformerConfig(
    name="facebook/opt-125m", family="opt", vocab_size=50272, hidden_size=768, num_layers=12,
    num_heads=12, ffn_size=3072, max_positions=2048, position_offset=2, activation="relu",
    pre_ln=True, causal=True, final_ln=True, ln_eps=1e-5, hidden_dropout=0.1, attn_dropout=0.0,
    pad_token_id=1, special_token_ids=(0, 1, 2),
)
GPT2_MEDIUM = TransformerConfig(
    name="gpt2-medium", family="gpt2", vocab_size=50257, hidden_size=1024, num_layers=24,
    num_heads=16, ffn_size=4096, max_positions=1024, activation="gelu_tanh", pre_ln=True,
    causal=True, final_ln=True, ln_eps=1e-5, hidden_dropout=0.1, attn_dropout=0.1,
    pad_token_id=50256, special_token_ids=(50256,),
)
# Estimator block of estimate_transformer_memory.py:59-69 (OPT-style, h=9216, a=72, ffn 4h).
W4_BLOCK = TransformerConfig(
    name="w4-block", family="block", vocab_size=0, hidden_size=9216, num_layers=1, num_heads=72,
    ffn_size=36864, max_positions=512, activation="relu", pre_ln=True, causal=False,
    ln_eps=1e-5, hidden_dropout=0.1, attn_dropout=0.1,
)
CAUSAL_TINY = GPT2_MEDIUM.with_(name="causal-tiny", vocab_size=1024, hidden_size=128,
                                num_layers=2, num_heads=2, ffn_size=512, max_positions=512)

# Llama family (HF LlamaForCausalLM): RMSNorm, rotary embeddings, SwiGLU MLP, no biases, no position
# table, untied head.  num_kv_heads < num_heads: grouped-query attention (TinyLlama, Llama-3).  Parameter
# counts (tests/test_llama_cpu.py, tests/test_gqa_cpu.py): 2 V h + L (2 h^2 + 2 h Hkv D + 3 h f + 2 h) + h,
# with Hkv D = h for multi-head attention; with E experts (Mixtral, below) the FFN term L 3 h f becomes
# L (E 3 h f + E h): E expert FFNs and the [E, h] router.  Mistral is a grouped-query Llama with sliding_window keys per
# query (HF MistralForCausalLM; the tensor names are Llama's).  Llama-3.1 / 3.2 (rotary scaling) are not
# described here.
LLAMA_160M = TransformerConfig(
    name="JackFram/llama-160m", family="llama", vocab_size=32000, hidden_size=768, num_layers=12,
    num_heads=12, ffn_size=3072, max_positions=2048, activation="swiglu", pre_ln=True, causal=True,
    final_ln=True, tie_word_embeddings=False, ln_eps=1e-6, hidden_dropout=0.0, attn_dropout=0.0,
    bias=False, pad_token_id=0, special_token_ids=(0, 1, 2), norm="rms", rope_theta=10000.0,
)
SHEARED_LLAMA_1_3B = LLAMA_160M.with_(name="princeton-nlp/Sheared-LLaMA-1.3B", hidden_size=2048, num_layers=24,
                                      num_heads=16, ffn_size=5504, max_positions=4096, ln_eps=1e-5)
LLAMA_2_7B = LLAMA_160M.with_(name="meta-llama/Llama-2-7b-hf", hidden_size=4096, num_layers=32, num_heads=32,
                              ffn_size=11008, max_positions=4096, ln_eps=1e-5)
LLAMA_TINY = LLAMA_160M.with_(name="llama-tiny", vocab_size=1024, hidden_size=128, num_layers=2, num_heads=2,
                              ffn_size=384, max_positions=512)
# grouped-query attention
TINYLLAMA_1_1B = LLAMA_160M.with_(name="TinyLlama/TinyLlama_v1.1", hidden_size=2048, num_layers=22, num_heads=32,
                                  num_kv_heads=4, ffn_size=5632, max_positions=2048, ln_eps=1e-5)
LLAMA_3_8B = LLAMA_160M.with_(name="meta-llama/Meta-Llama-3-8B", vocab_size=128256, hidden_size=4096, num_layers=32,
                              num_heads=32, num_kv_heads=8, ffn_size=14336, max_positions=8192, ln_eps=1e-5,
                              rope_theta=500000.0)
LLAMA_TINY_GQA = LLAMA_160M.with_(name="llama-tiny-gqa", vocab_size=1024, hidden_size=256, num_layers=2, num_heads=4,
                                  num_kv_heads=2, ffn_size=768, max_positions=512)
# sliding window
MISTRAL_7B = LLAMA_160M.with_(name="mistralai/Mistral-7B-v0.1", hidden_size=4096, num_layers=32, num_heads=32,
                              num_kv_heads=8, ffn_size=14336, max_positions=32768, ln_eps=1e-5, sliding_window=4096)
MISTRAL_TINY = LLAMA_TINY_GQA.with_(name="mistral-tiny", sliding_window=48)
# mixture of experts (HF MixtralForCausalLM): Mistral's attention without the window, E SwiGLU experts per
# layer, k of them per token.  mixtral-8x7b (46,702,792,704 parameters) is described and counted, not trained
# on one card.
MIXTRAL_8X7B = MISTRAL_7B.with_(name="mistralai/Mixtral-8x7B-v0.1", sliding_window=0, rope_theta=1e6, num_experts=8,
                                experts_per_token=2, router_aux_loss_coef=0.02)
MOE_8X160M = LLAMA_160M.with_(name="moe-8x160m", num_experts=8, experts_per_token=2, router_aux_loss_coef=0.02)
MIXTRAL_TINY = LLAMA_TINY_GQA.with_(name="mixtral-tiny", num_experts=4, experts_per_token=2,
                                    router_aux_loss_coef=0.02)

PRESETS = {
    c.name: c
    for c in (BERT_BASE, BERT_LARGE, BERT_TINY, BLOOM_560M, OPT_125M, GPT2_MEDIUM, W4_BLOCK,
              CAUSAL_TINY, LLAMA_160M, SHEARED_LLAMA_1_3B, LLAMA_2_7B, LLAMA_TINY, TINYLLAMA_1_1B, LLAMA_3_8B,
              LLAMA_TINY_GQA, MISTRAL_7B, MISTRAL_TINY, MIXTRAL_8X7B, MOE_8X160M, MIXTRAL_TINY)
}
ALIASES = {
    "base": "bert-base-cased", "large": "bert-large-cased", "tiny": "bert-tiny",
    "bert-base": "bert-base-cased", "bert-large": "bert-large-cased",
    "bloom-560m": "bigscience/bloom-560m", "opt-125m": "facebook/opt-125m",
    "openai-community/gpt2-medium": "gpt2-medium",
    "llama-160m": "JackFram/llama-160m", "sheared-llama-1.3b": "princeton-nlp/Sheared-LLaMA-1.3B",
    "llama-2-7b": "meta-llama/Llama-2-7b-hf",
    "tinyllama-1.1b": "TinyLlama/TinyLlama_v1.1", "llama-3-8b": "meta-llama/Meta-Llama-3-8B",
    "mistral-7b": "mistralai/Mistral-7B-v0.1", "mixtral-8x7b": "mistralai/Mixtral-8x7B-v0.1",
}


def get_config(name: str | TransformerConfig) -> TransformerConfig:
    """The preset of that name or alias; a ``TransformerConfig`` (a preset altered with ``with_``) is
    returned as it is, so whatever takes a preset's name takes such a config too."""
    if isinstance(name, TransformerConfig):
        return name
    key = ALIASES.get(name, name)
    if key not in PRESETS:
        raise KeyError(f"unknown model preset {name!r}; known: {sorted(PRESETS) + sorted(ALIASES)}")
    return PRESETS[key]
