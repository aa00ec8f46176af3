"""The S2+DSM model with BiLSTM fusion, behind the reference's module names
(reference: pretraining/multimae/multimae_lstm_s2dsm.py -- class MultiMAE :37-502, factories :505-557; driver
pretraining/pretrain_mmae_s2dsm.py:181-241, step :440-500).

The quadruplet-style encoder (Zorro-masked Block stack, no Block_Fusion, no mask_embedding, no per-modality contrastive tokens)
on the packed pipeline of multimae_crossattn.MultiMAE, with the reference's four changes:
  * N fusion rows, one per kept modality token j: fusion_tokens[patch_j] + fusion pos-emb[patch_j] (:408, :421);
    row space per step [ B*N modality tokens | B*N fusion rows ];
  * before the first block, every pair (token j, fusion row j) goes through AttentionBiLSTM (ops.bilstm2_attn_pool, csrc/bilstm.hip)
    and its result replaces fusion row j (:428-434);
  * Zorro mask: a modality attends its own rows, fusion rows attend every row of the sample (:415-424) -- the header's segment rule
    with the last segment at the sample's fusion rows; the pool rule (:459-463) is the same one;
  * the decoders read the (B, P, D) fusion grid: the normalised encoder fusion row of the LAST modality keeping the patch, else
    the un-normalised learned token (:473-476, ops.last_wins_fusion).
Forward returns (preds, task_masks, return_tokens (B,3,D), ori_tokens (B,N,D), encoder_fusion_tokens (B,N,D)) (:502), or
(tokens (B,2N,D), return_tokens, task_masks) without output adapters (:466-467).  State-dict keys, shapes and order are the
reference's (tests/golden/s2dsm_tiny.npz).

Shared with multimae_crossattn.MultiMAE (defined there once): the constructor prologue, input validation, masks -> descriptors,
patch embedding of the kept patches, attention pooling, the decoder loop, mask generation, make_mask and no_weight_decay.  Owned
here: the rest of the constructor (the reference's registration order: ..., mlp, attn_lstm, blocks, norm), the BiLSTM fusion
stage, the encoder Segments, the Block loop, the final norm, the last-wins rows handed to the decoders, the return tuples.
"""
from typing import Dict, List, Optional, Tuple, Union

import torch
from torch import nn

from .. import ops
from . import multimae_crossattn as _mc
from .zorro_utils import AttentionBiLSTM, Block, LayerNorm, Mlp, TokenTypes, linear

__all__ = ['pretrain_multimae_tiny', 'pretrain_multimae_base', 'pretrain_multimae_large', 'MultiMAE']


class MultiMAE(_mc.MultiMAE):
    """The shared stages, mask generation, make_mask and no_weight_decay are multimae_crossattn.MultiMAE's; its own constructor
    (the reference's registration order: ..., mlp, attn_lstm, blocks, norm) and forward."""

    def __init__(self, input_adapters: Dict[str, nn.Module], output_adapters: Optional[Dict[str, nn.Module]],
                 num_global_tokens: int = 1, dim_tokens: int = 768, depth: int = 12, dim_head: int = 64, heads: int = 8,
                 ff_mult: int = 4, num_fusion_tokens: int = 16,
                 return_token_types: Tuple[TokenTypes] = (TokenTypes.S1, TokenTypes.S2, TokenTypes.DEM, TokenTypes.FUSION),
                 drop_path_rate: float = 0.0, norm_layer: nn.Module = LayerNorm):
        nn.Module.__init__(self)
        assert num_fusion_tokens == input_adapters['s2'].num_patches                   # reference :87
        domains = ['s2', 'dem']                                                        # the token order of :402-407
        for d in domains:
            assert d in input_adapters, "the S2+DSM model needs the 's2' and 'dem' input adapters"
        # pool rule on the device: return token i attends modality segment i (S2 rows, DEM rows), the last one every row -- the
        # reference's rule for (S2, DEM, FUSION) = (1, 2, 3) against token types (S2, DEM, FUSION) (:459-463)
        names = [t.name for t in return_token_types]
        assert names == ['S2', 'DEM', 'FUSION'], "return_token_types must be (S2, DEM, FUSION) (pretrain_mmae_s2dsm.py:236)"
        self._init_shared(input_adapters, output_adapters, domains, dim_tokens, depth, dim_head, heads, num_fusion_tokens,
                          return_token_types)
        self.mlp = Mlp(in_features=dim_tokens, hidden_features=int(dim_tokens * 4.0))
        self.attn_lstm = AttentionBiLSTM(dim_tokens)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([
            Block(dim=dim_tokens, dim_head=dim_head, heads=heads, ff_mult=ff_mult, drop_path=dpr[i], norm_layer=norm_layer)
            for i in range(depth)])
        self.norm = LayerNorm(dim_tokens)
        self.has_fusion_blocks, self.has_contrastive_tokens = False, False
        self._reset_parameters()          # xavier on every Linear, Attention_LSTM's included (reference :134-146)

    def never_used_parameters(self):
        """Every decoder's task embeddings of OTHER tasks (output_adapters_simple.py:172-174).  Unlike the DINO-trained models, the
        pooled `return_tokens` are trained here: the driver's hard-negative loss reads the pooled tokens (:482-492)."""
        return [p for p in super().never_used_parameters() if p is not self.return_tokens]

    def _encode(self, x, doms, desc, taps=()):
        raise NotImplementedError("the S2+DSM model has no downstream encoder path here")

    def forward(self,
                x: Union[Dict[str, torch.Tensor], torch.Tensor],
                mask_inputs: bool = True,
                task_masks: Dict[str, torch.Tensor] = None,
                num_encoded_tokens: int = 128,
                alphas: Union[float, List[float]] = 1.0,
                sample_tasks_uniformly: bool = False,
                fp32_output_adapters: List[str] = [],
                return_token_indices: Optional[Tuple[int]] = None):
        x, B, H, W, P, N, T = self._begin(x, 's2', mask_inputs, num_encoded_tokens, return_token_indices)
        doms = self.domains
        M, D, Hh, dh = len(doms), self.dim_tokens, self.heads, self.dim_head
        device = x['s2'].device
        task_masks, desc = self._descriptors(x, doms, N, task_masks, alphas, sample_tasks_uniformly)
        BN = B * N
        tok, pe = self._embed_kept(x, doms, desc)
        xm = pe + tok.float()                                                                # s2 / dem tokens (:392-407)

        # -- fusion rows: the learned token at each kept token's patch (:408), then the BiLSTM fusion (:428-434) ------------
        learned = (self.fusion_tokens[0] + self.input_adapters['fusion'].posemb_rows()).contiguous()      # (P, D) fp32
        grid = learned.unsqueeze(0).expand(B, P, D).reshape(B * P, D)
        # token j of sample b reads grid row b*P + patch_j: unique within one modality (ops.gather_rows' class filter)
        xf0 = ops.gather_rows(grid, desc.tok_fus - BN, unique=False, filt=desc.tok_mod, nfilt=M)
        xf = self.attn_lstm.pool_pairs(xm, xf0)                                               # (B*N, D) fp32

        # -- encoder segments: the modality segments of the descriptors, the fusion segment at B*N + b*N --------------------
        fus_start = (BN + N * torch.arange(B, dtype=torch.int32, device=device)).unsqueeze(1)
        seg = ops.Segments(torch.cat([desc.enc_start[:, :M], fus_start], dim=1),
                           torch.cat([desc.enc_len[:, :M], desc.enc_len[:, :M].sum(dim=1, keepdim=True, dtype=torch.int32)],
                                     dim=1), 2 * N)

        # -- Zorro-masked Block stack (:436-438) ------------------------------------------------------------------------------
        dl = None
        for blk in self.blocks:
            (xm, xf), z = ops.parts_add_ln([xm, xf], dl, [0, BN] if dl is not None else [-1, -1], blk.norm1.gamma, None,
                                           blk.attn.norm.gamma, None, out_dtype=T)                 # (2BN, D)
            qkv = linear(z, [blk.attn.to_q.weight, blk.attn.to_kv.weight], once=True)
            a = ops.mha_self(qkv, Hh, dh, seg, blk.attn.scale)
            o = blk.drop_rows(linear(a, blk.attn.to_out.weight, once=True), B, (N, N))
            (xm, xf), y = ops.parts_add_ln([xm, xf], o, [0, BN], blk.norm2.gamma, None, blk.mlp[0].gamma, None, out_dtype=T)
            dl = blk.drop_rows(ops.feedforward_geglu(y, blk.mlp[1].weight, blk.mlp[3].weight), B, (N, N))

        # -- final norm (:440) --------------------------------------------------------------------------------------------------
        (xm, xf), tokens = ops.parts_add_ln([xm, xf], dl, [0, BN] if dl is not None else [-1, -1], self.norm.gamma, None,
                                            out_dtype=torch.float32)
        tokens_T = tokens if T == torch.float32 else tokens.to(T)
        ori_tokens = tokens[:BN].reshape(B, N, D)                                             # :465
        enc_fus = tokens[BN:].reshape(B, N, D)                                                # :470

        # -- attention pooling into the return tokens (:442-464) ----------------------------------------------------------
        kvp = linear(tokens_T, self.attn_pool.to_kv.weight, once=True)                       # (2BN, 2I)
        return_tokens = self._attn_pool(self.return_tokens[0].contiguous(), kvp, desc.pool_q, seg, B, 0, return_token_indices)

        if self.output_adapters is None:
            return tokens.reshape(2, B, N, D).transpose(0, 1).reshape(B, 2 * N, D), return_tokens, task_masks   # :466-467

        # -- decoders on the (B, P, D) fusion grid, last write wins (:473-498): one grid per output adapter, from the fp32
        # tokens for an fp32 adapter
        def fusion_grid(fp32):
            return ops.last_wins_fusion((tokens if fp32 else tokens_T)[BN:], learned, desc.slot_row, B, P, M, BN)
        preds = self._decode(B, H, W, fusion_grid, fp32_output_adapters)
        return preds, task_masks, return_tokens, ori_tokens, enc_fus                          # :502


pretrain_multimae_tiny = _mc._factory(MultiMAE, 192, 12, 3)      # reference :505-520 (the driver's choice, pretrain_mmae_s2dsm.py:231)
pretrain_multimae_base = _mc._factory(MultiMAE, 768, 12, 8)      # :523-538
pretrain_multimae_large = _mc._factory(MultiMAE, 1024, 24, 8)    # :541-557
