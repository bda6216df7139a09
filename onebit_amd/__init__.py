"""onebit_amd -- MI355X-native implementation of OneBit's 1-bit linear inference path.

Public surface mirrors the reference's for this path:
  BitLinearInf / OneBitLinear   drop-in nn.Module (reference: models/bitnet.py:71-122)
  fp16_to_int8 / pack_signs     sign packer (reference: scripts/convert_llama_to_infer_ckpt.py:7-15)
  int8_to_fp16                  unpacker (reference: models/bitnet.py:98-110)
  KDLoss / kd_token_loss / kd_hidden_loss   knowledge-distillation objective (reference: llamafactory/kd.py:34-113)
  svid_decompose / build_start_state_dict / build_inference_state_dict   SVID start checkpoints from a teacher
                                (reference: scripts/build_start_ckpt.py)
  OneBitLlamaForCausalLMTrain / flash_attention_train   the train-mode model on train.BitLinear and its causal attention with
                                a flash-style HIP forward and backward (reference: modeling_bitllama.py BitLlamaForCausalLM)
"""
from .bitnet import BitLinearInf, OneBitLinear, fp16_to_int8, int8_to_fp16, pack_signs  # noqa: F401
from .kd import KDLoss, kd_hidden_loss, kd_token_loss  # noqa: F401
from .svid import (SvidResult, build_inference_state_dict, build_start_state_dict, svid_decompose, svid_init,  # noqa: F401
                   svid_start_layer)
from .train_model import OneBitLlamaForCausalLMTrain, eager_attention_train, flash_attention_train  # noqa: F401

__version__ = "0.1.0"
