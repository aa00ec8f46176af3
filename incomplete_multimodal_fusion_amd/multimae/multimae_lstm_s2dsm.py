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
"""
from typing import Dict, List, Optional, Tuple, Union

import torch
from torch import nn

from .. import ops
from . import multimae_crossattn as _mc
from .input_adapters import interp_posemb
from .multimae_utils import trunc_normal_
from .zorro_utils import Attention, AttentionBiLSTM, Block, LayerNorm, Mlp, TokenTypes, compute_dtype, exists, linear

__all__ = ['pretrain_multimae_tiny', 'pretrain_multimae_base', 'pretrain_multimae_large', 'MultiMAE']


class MultiMAE(_mc.MultiMAE):
    """Shares mask generation, make_mask, no_weight_decay and the behaviour switches with multimae_crossattn.MultiMAE; its own
    constructor (the reference's registration order: ..., mlp, attn_lstm, blocks, norm) and forward."""

    def __init__(self, input_adapters: Dict[str, nn.Module], output_adapters: Optional[Dict[str, nn.Module]],
                 num_global_tokens: int = 1, dim_tokens: int = 768, depth: int = 12, dim_head: int = 64, heads: int = 8,
                 ff_mult: int = 4, num_fusion_tokens: int = 16,
                 return_token_types: Tuple[TokenTypes] = (TokenTypes.S1, TokenTypes.S2, TokenTypes.DEM, TokenTypes.FUSION),
                 drop_path_rate: float = 0.0, norm_layer: nn.Module = LayerNorm):
        nn.Module.__init__(self)
        for adapter in input_adapters.values():
            adapter.init(dim_tokens=dim_tokens)
        self.input_adapters = nn.ModuleDict(input_adapters)
        if output_adapters is not None:
            for adapter in output_adapters.values():
                adapter.init(dim_tokens_enc=dim_tokens)
            self.output_adapters = nn.ModuleDict(output_adapters)
        else:
            self.output_adapters = None
        assert num_fusion_tokens == input_adapters['s2'].num_patches                   # reference :87
        self.domains = ['s2', 'dem']                                                   # the token order of :402-407
        for d in self.domains:
            assert d in input_adapters, "the S2+DSM model needs the 's2' and 'dem' input adapters"
        self.dim_tokens, self.depth, self.heads, self.dim_head = dim_tokens, depth, heads, dim_head
        self.max_return_tokens = len(return_token_types)
        self.return_token_types = return_token_types
        self.register_buffer('return_token_types_tensor',
                             torch.tensor([t.value for t in return_token_types]), persistent=False)
        # pool rule on the device: return token i attends modality segment i (S2 rows, DEM rows), the last one every row -- the
        # reference's rule for (S2, DEM, FUSION) = (1, 2, 3) against token types (S2, DEM, FUSION) (:459-463)
        names = [t.name for t in return_token_types]
        assert names == ['S2', 'DEM', 'FUSION'], "return_token_types must be (S2, DEM, FUSION) (pretrain_mmae_s2dsm.py:236)"

        self.return_tokens = nn.Parameter(trunc_normal_(torch.zeros(1, self.max_return_tokens, dim_tokens), std=0.02))
        self.attn_pool = Attention(dim=dim_tokens, dim_head=dim_head, heads=heads)
        self.fusion_tokens = nn.Parameter(trunc_normal_(torch.zeros(1, num_fusion_tokens, dim_tokens), std=0.02))
        self.mlp = Mlp(in_features=dim_tokens, hidden_features=int(dim_tokens * 4.0))
        self.attn_lstm = AttentionBiLSTM(dim_tokens)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([
            Block(dim=dim_tokens, dim_head=dim_head, heads=heads, ff_mult=ff_mult, drop_path=dpr[i], norm_layer=norm_layer)
            for i in range(depth)])
        self.norm = LayerNorm(dim_tokens)
        self.has_fusion_blocks, self.has_contrastive_tokens = False, False

        # behaviour switches of the native path (not part of the reference API; see multimae_crossattn.MultiMAE)
        self.per_sample_masks = False      # True: every sample uses its own mask row (the reference uses row 0 for the batch)
        self.fuse_unpatchify_loss = False
        self.check_masks = True
        self.side_stream_wgrad = False
        self.decoder_streams = False
        self._dec_streams = []
        self.layer_timer = None

        self._reset_parameters()           # xavier on every Linear, Attention_LSTM's included (reference :134-146)

    def never_used_parameters(self):
        """Every decoder's task embeddings of OTHER tasks (output_adapters_simple.py:172-174).  Unlike the DINO-trained models, the
        pooled `return_tokens` are trained here: the driver's hard-negative loss reads the pooled tokens (:482-492)."""
        return [p for p in super().never_used_parameters() if p is not self.return_tokens]

    def _encode(self, x, doms, mask_all, N, explicit, taps=()):
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
        x = {'s2': x} if isinstance(x, torch.Tensor) else x
        B, _, H, W = x['s2'].shape
        device = x['s2'].device
        doms = self.domains
        for d in doms:
            _ = x[d]
        if exists(return_token_indices):
            assert len(set(return_token_indices)) == len(return_token_indices), 'all indices must be unique'
            assert all(i < self.max_return_tokens for i in return_token_indices), \
                'indices must range from 0 to max_num_return_tokens - 1'
        M, D, Hh, dh = len(doms), self.dim_tokens, self.heads, self.dim_head
        ps = self.input_adapters[doms[0]].P_H
        nh, nw = H // ps, W // ps
        P = nh * nw
        assert P == self.fusion_tokens.shape[1], "fusion tokens are tied to the patch grid (reference :87)"
        T = compute_dtype(self.fusion_tokens)
        N = num_encoded_tokens if mask_inputs else M * P

        # -- masks + device-side descriptors --------------------------------------------------------------------------------
        if task_masks is None:
            placeholders = {d: torch.empty(B, P, 0, device=device) for d in doms}
            task_masks, _, _ = self.generate_random_masks(placeholders, N, alphas=alphas,
                                                          sample_tasks_uniformly=sample_tasks_uniformly)
            mask_all = torch.cat([task_masks[d][:(B if self.per_sample_masks else 1)] for d in doms], dim=1)
            explicit = False
        else:
            mask_full = torch.cat([task_masks[d] for d in doms], dim=1).to(torch.int64)
            mask_all = mask_full if self.per_sample_masks else mask_full[:1]      # row 0 drives the batch (:402-406)
            explicit = True
        desc = ops.Descriptors(mask_all.contiguous(), B, M, P, N)
        if explicit and self.check_masks:
            desc.check()
        BN = B * N

        # -- patch embedding of the kept patches (one gather + one GEMM, as multimae_crossattn) + pos-emb ------------------
        Ks = [self.input_adapters[d].packed_channels * ps * ps for d in doms]
        koff = [sum(Ks[:i]) for i in range(M)]
        onehot = sum(Ks)
        Kcat = onehot + ((M + 7) // 8) * 8
        pcat = ops.patchify_gather([self.input_adapters[d].packed_image(x[d]) for d in doms], koff, onehot, Kcat, ps,
                                   desc.tok_mod, desc.tok_patch, N, T)
        wcat = torch.cat([self.input_adapters[d].packed_weight() for d in doms] +
                         [torch.stack([self.input_adapters[d].packed_bias() for d in doms], dim=1),
                          pcat.new_zeros(D, Kcat - onehot - M, dtype=torch.float32)], dim=1)
        tok = linear(pcat, wcat, once=True)                                                   # (B*N, D), bias included
        pe_table = torch.cat([interp_posemb(self.input_adapters[d].pos_emb, nh, nw) for d in doms], dim=0)
        if pe_table.requires_grad:
            pe = pe_table.index_select(0, desc.tok_pe.long())
        else:
            pe = ops.gather_rows(pe_table.detach().contiguous(), desc.tok_pe)
        xm = pe + tok.float()                                                                 # s2 / dem tokens (:392-407)

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
        ap = self.attn_pool
        R = self.max_return_tokens
        kvp = linear(tokens_T, ap.to_kv.weight, once=True)                                   # (2BN, 2I)
        rq = linear(ops.layernorm(self.return_tokens[0].contiguous(), ap.norm.gamma, out_dtype=T), ap.to_q.weight)
        a = ops.mha_cross(rq.repeat(B, 1), kvp, Hh, dh, desc.pool_q, seg, ap.scale, empty_mode=0)
        pooled = linear(a, ap.to_out.weight).float()                                          # (B*R, D)
        pooled = pooled + self.mlp(ops.layernorm(pooled, self.norm.gamma, out_dtype=T)).float()
        return_tokens = pooled.reshape(B, R, D)
        if exists(return_token_indices):
            return_tokens = return_tokens[:, torch.tensor(list(return_token_indices), dtype=torch.long, device=device)]

        if self.output_adapters is None:
            return tokens.reshape(2, B, N, D).transpose(0, 1).reshape(B, 2 * N, D), return_tokens, task_masks   # :466-467

        # -- decoders on the (B, P, D) fusion grid, last write wins (:473-498) --------------------------------------------
        dec_seg = ops.Segments.dense(B, P, device)
        preds = {}
        for d, adapter in self.output_adapters.items():
            if d in fp32_output_adapters:
                rows = ops.last_wins_fusion(tokens[BN:], learned, desc.slot_row, B, P, M, BN)
                with torch.autocast("cuda", enabled=False):
                    tk = adapter.forward_tokens(rows, B, P, dec_seg, once=True)
            else:
                rows = ops.last_wins_fusion(tokens_T[BN:], learned, desc.slot_row, B, P, M, BN)
                tk = adapter.forward_tokens(rows, B, P, dec_seg, once=True)
            C = adapter.num_channels
            preds[d] = _mc.PredTokens(tk, B, C, H, W, adapter.P_H) if self.fuse_unpatchify_loss else \
                ops.unpatchify(tk, B, C, H, W, adapter.P_H)
        return preds, task_masks, return_tokens, ori_tokens, enc_fus                          # :502


def _factory(dim_tokens, depth, heads):
    def build(input_adapters: Dict[str, nn.Module], output_adapters: Optional[Dict[str, nn.Module]], **kwargs):
        return MultiMAE(input_adapters=input_adapters, output_adapters=output_adapters, dim_tokens=dim_tokens, depth=depth,
                        dim_head=64, heads=heads, ff_mult=4, norm_layer=LayerNorm, **kwargs)
    return build


pretrain_multimae_tiny = _factory(192, 12, 3)      # reference :505-520 (the driver's choice, pretrain_mmae_s2dsm.py:231)
pretrain_multimae_base = _factory(768, 12, 8)      # :523-538
pretrain_multimae_large = _factory(1024, 24, 8)    # :541-557
