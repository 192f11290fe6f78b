"""PFCN_MLP: PFCN on an MLP scorer over cat(user, item) (reference: recbole/model/fair_recommender/pfcn_mlp.py).
Tables are named `user_embedding` / `item_embedding`, the scorer `mlp_layer` (registered, trained by optimizer_filter)."""
import torch

from ..layers import MLPLayers, full_sort_pair_mlp_pieces, full_sort_scorer_of
from .pfcn_base import PFCNBase


class PFCN_MLP(PFCNBase):
    biased = False
    user_table_attr = "user_embedding"
    item_table_attr = "item_embedding"

    def _build_base_layers(self, config):
        self.full_sort_scorer = full_sort_scorer_of(config)
        self.dropout = config['dropout']
        self.mlp_hidden_size_list = config['mlp_hidden_size_list']
        self.mlp_layer = MLPLayers([self.embedding_size * 2] + list(self.mlp_hidden_size_list) + [1], dropout=self.dropout)

    def _base_dense_modules(self):
        return {"mlp_layer": self.mlp_layer}

    def _score(self, user_embed, item_embed):          # pfcn_mlp.py:185-186, [B, 1]; BPR then averages over B
        return self.mlp_layer(user_embed, item_embed).view(-1)

    def _predict_score(self, ue, ie):
        return self.mlp_layer(ue, ie)

    def full_sort_pair_mlp(self, interaction, sst_list=None, users_per_batch=None):
        """The pieces of predict() on every item for fr_pair_mlp_scores (`full_sort_scorer: split`), or None: the dense path
        then serves the call.  The users go through the filters as in PFCNBase.full_sort_factors: `users_per_batch` at a time
        under batch statistics (the users of one predict() batch of the full-sort evaluation), in any grouping under
        `filter_eval_statistics: running`."""
        if self.shard is not None:
            return None
        eng = self.hip_engine()

        def user_rows():
            ue = eng.lookup(self._utab, interaction[self.USER_ID])
            if self.filter_mode != 'none' and ue.shape[0]:
                per = int(users_per_batch) if users_per_batch else ue.shape[0]
                ue = torch.cat([self._filter(ue[lo:lo + per], sst_list) for lo in range(0, ue.shape[0], per)])
            return ue

        return full_sort_pair_mlp_pieces(self.full_sort_scorer, self.mlp_layer, eng, user_rows, self._itab, self.n_items)
