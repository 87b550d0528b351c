"""The compressed container of `Compressor2018.compress` / `decompress` (and of
`MeanScaleCompressor2018`'s), and the specification of the rANS bitstream inside it (kernels:
csrc/codec.hip and csrc/meancodec.hip, `ic_codec_*`).  Host code only: nothing
here launches a kernel, and `parse` validates a buffer completely before the caller launches any.

Bitstream of one tensor
-----------------------
Symbols.  The tensor's eval-mode quantization q = rint(x) as integers, flattened in (n, h, w, c)
order (channel fastest).  K = kmax = max |q| of the tensor, K <= 2047; symbol index j = q + K in
[0, 2K].
With the mean-scale hyperprior (conditional kind 2 or 3 below) the symbols of y are those of the residual,
q = rint(y - mu) with y - mu one float32 subtraction, where (mu, sigma) = h_s(z_hat) are computed from the decoded
integers of z; K is the largest |residual|, and the decoder's reconstruction is y_hat = q + mu, one float32
addition.  The symbols of z, the tables, the rows, the chunks and the payload are unchanged: the rows of y are pmfs
at mean 0, which is what the residual is coded under.

Tables.  A table has `rows` rows of 2K+2 unsigned cumulative counts: cdf[0] = 0 < cdf[1] < ... <
cdf[2K+1] = 65536.  Symbol j has start = cdf[j], freq = cdf[j+1] - cdf[j] >= 1.  The row of symbol
number i (its position in the flattened tensor) is i % C for z (one row per channel: the factorized
prior) and index(sigma_i) for y, where index(s) = the number of midpoints strictly below s, the
midpoints being m_t = float32(sqrt(S_t * S_{t+1})) of the L log-spaced scales
S_t = exp(ln(scale_min) + t * (ln(scale_max) - ln(scale_min)) / (L - 1)) computed in float64, and the
comparison s > m_t made in float32.  Row t of the y table is the conditional model's pmf at scale
float32(S_t).  How a pmf becomes counts is DESIGN.md's table rule; the coder only needs the
properties above.

Chunks.  The symbols are cut into chunks of 64 * R consecutive symbols (R = steps_per_chunk; the last
chunk may be shorter).  Symbol i of a chunk (i counted from the chunk's first symbol) belongs to
lane i % 64 and step i // 64; the last step of a chunk may hold fewer than 64 symbols (lanes
0 .. m-1).  Each lane is an independent rANS coder: 32-bit state x in [2^16, 2^32), precision 16,
16-bit renormalisation words.

Encoding a chunk.  Every lane starts at x = 2^16.  Steps are taken from the last to the first.  At a
step, a lane that holds a symbol (start, freq):
    if x >= freq * 2^16:  emit the word x & 0xFFFF;  x >>= 16          (at most once)
    x = (x // freq) * 2^16 + (x % freq) + start
Decoding reads the words forward, so the word sequence of a chunk is defined by the decoder's order:
ascending step, and within a step ascending lane among the lanes that emitted at that step.  (The
encoder, running backwards, fills its buffer from the end.)

Chunk bytes.  64 final encoder states as little-endian uint32, lane 0 first (256 bytes, the fixed
cost per chunk, written for idle lanes too), then the words as little-endian uint16 in the order
above.  A chunk's length is 256 + 2 * (number of words) bytes, at most 256 + 2 * 64 * R.

Decoding a chunk.  Lane l starts at the l-th state.  Steps ascend; at a step a lane that holds a
symbol:
    slot = x & 0xFFFF;  j = the index with cdf[j] <= slot < cdf[j+1] in the symbol's row
    x = freq * (x >> 16) + slot - start
    if x < 2^16:  x = (x << 16) | next word                            (at most once)
where the lanes that refill at a step take consecutive words in ascending lane order.  A word past
the chunk's end reads as 0.  The symbol is q = j - K.

Payload.  The chunks back to back, in order; the chunk lengths are kept beside it (uint32 each).

Container (little endian), one call = one batch = one bytes object
-------------------------------------------------------------------
    magic "ICRA", u16 format version (1), u8 arithmetic tag (index of COMPUTE_DTYPE in
    COMPUTE_DTYPES), u8 conditional kind (bit 0: 0 Laplace, 1 Gauss; bit 1 set: y is coded about a mean
    from h_s, the mean-scale hyperprior; so 0..3, anything else is rejected), u32 ABI version (ic_version()),
    u32 N, H, W (image batch), u32 latent channels (y), u32 hyper channels (z),
    u32 L, f64 scale_min, f64 scale_max, u32 R, u32 kmax_z, u32 kmax_y,
    u64 symbols of z, u64 symbols of y, u32 chunks of z, u32 chunks of y,
    chunk lengths of z (u32 each), chunk lengths of y, payload of z, payload of y.
y has N x latent x H/16 x W/16 symbols, z N x hyper x H/64 x W/64.

Per-image container (little endian), one image = one bytes object (`compress_each`)
------------------------------------------------------------------------------------
An image of any size h x w >= 1 is padded at the bottom and the right to H = 64 * ceil(h / 64),
W = 64 * ceil(w / 64) by replicating its last row and column, x_pad[c, i, j] = x[c, min(i, h-1),
min(j, w-1)], and the padded image is coded; the decoder returns the top-left h x w of the
reconstruction.  The two bitstreams are exactly the ones above for a batch of one: symbols of this
image only in (h, w, c) order, K = the largest |symbol| of this image's tensor, chunks cut from the
image's first symbol (no chunk holds symbols of two images), and the rows of y from
sigma = h_s(z_hat) evaluated on this image alone (batch shape 1), whoever else is coded or decoded in
the same call (with kind 2 or 3, mu comes from the same single-image evaluation).
    magic "ICRP", u16 format version (1), then the fields of the "ICRA" header from the arithmetic
    tag to the chunk counts, with N = 1 and H, W the padded size,
    u32 image height h, u32 image width w   (1 <= h <= H, H - h < 64; 1 <= w <= W, W - w < 64),
    chunk lengths of z (u32 each), chunk lengths of y, payload of z, payload of y.

Checkerboard container (little endian), one call = one batch = one bytes object (`CheckerboardCompressor2018`)
--------------------------------------------------------------------------------------------------------------
y is coded in two passes.  Position (i, j) of a latent map is an anchor when i + j is even (the parity does not
depend on n or c).  With (sigma_h, mu_h) = h_s(z_hat): the anchors are coded as above for kind 2 or 3, symbols
rint(y - mu_h), rows index(sigma_h).  From the decoded anchors y_hat = q + mu_h the context model gives every
non-anchor its own (sigma, mu) (modelling/meta_arch/ckbd2021.py `_context`), and the non-anchors are coded with symbols
rint(y - mu), rows index(sigma), reconstruction q + mu.  Each half is a bitstream of its own exactly as specified above:
the symbols of its positions in ascending (n, i, j, c) order, chunks cut from the half's first symbol.  One K = kmax_y
(the largest |symbol| of both halves) and so one table set serve both.
    magic "ICRC", u16 format version (1 or 2), then the fields of the "ICRA" header from the arithmetic tag to
    u64 symbols of y (the conditional kind is 2 or 3: 0 and 1 are rejected),
    u32 chunks of z, u32 chunks of the anchors of y, u32 chunks of the non-anchors of y,
    chunk lengths of z (u32 each), of the anchors, of the non-anchors, payload of z, of the anchors, of the non-anchors.
H and W are multiples of 64, so each half holds half of y's symbols.  The three containers do not read one another:
every parser raises ValueError on another's magic.
The format version names the arithmetic that gave the non-anchors their (sigma, mu), which the decoder must repeat bit
for bit: 1 -- the two context convs through the conv plans, in the model's COMPUTE_DTYPE (MODEL.CONTEXT.KERNEL "conv");
2 -- the fused context kernel, exact fp32 and independent of the batch (MODEL.CONTEXT.KERNEL "fused",
csrc/ckbd_context.hip).  The layout is the same; a model reads only the version it writes, and refuses the other by the
format-version error before any launch.

The route of h_s (every container)
----------------------------------
(sigma, mu) = h_s(z_hat) selects the table row of every symbol of y, so the decoder must repeat h_s bit for bit.  Every
container's format version says which route computed it, and a model reads only the version it writes:
    MODEL.HYPER_SYNTHESIS.KERNEL "conv" (default): the transposed convs through the conv plans, in the model's
        COMPUTE_DTYPE; a per-image path runs them one image at a time.  Version 1 ("ICRC": 1 or 2, by the context).
    MODEL.HYPER_SYNTHESIS.KERNEL "invariant": one launch per layer of csrc/hs_invariant.hip, once for all images of a
        call.  Version 2 (INVARIANT_FORMAT_VERSION; "ICRC": 3 or 4, by the context).  The layouts are the same.
The decodability contract's clause for "invariant": every layer output is one chain of fp32 fmaf (exact products, fp32
accumulation, fp32 MFMA) that starts from the bias and adds, in this order, the live taps (ky, kx) of the output's phase
(i % s, j % s) ascending; inside a tap the channel groups of 8 ascending; inside a group the channels +0, +4, +1, +5,
+2, +6, +3, +7; a tap outside the map and a channel past Cin add a product with +0.0.  The order is a function of
(k, s, Cin) only -- not of N, H, W, the image's index or the position's place in the map -- K is never split and there
are no atomics.  ReLU is x > 0 ? x : (x != x ? x : 0); sigma = fminf(fmaxf(expf(v), 1e-10), 1e10).  Every pack_* /
parse_* pair takes `version=` (default: the "conv" number; pack_checkerboard / parse_checkerboard keep `version` for
the context's route and take `invariant=` beside it).

Per-image checkerboard container (little endian), one image = one bytes object (`compress_each` of a "fused" model)
--------------------------------------------------------------------------------------------------------------------
The image is padded as for "ICRP" and its padded form coded as a checkerboard batch of one: h_s on this image alone,
the context from the fused kernel (whose result for an image does not depend on what else is in the call), K = the
largest |symbol| of this image's y over both halves, each half's chunks cut from the half's first symbol of this image.
    magic "ICRK", u16 format version (1), then the fields of the "ICRP" header from the arithmetic tag to
    u64 symbols of y, with N = 1, H, W the padded size and the conditional kind 2 or 3,
    u32 chunks of z, u32 chunks of the anchors of y, u32 chunks of the non-anchors of y,
    u32 image height h, u32 image width w   (as in "ICRP"),
    chunk lengths of z (u32 each), of the anchors, of the non-anchors, payload of z, of the anchors, of the non-anchors.

Gained containers (little endian): `GainedMeanScaleCompressor2018`, one network for a ladder of rates
------------------------------------------------------------------------------------------------------
The model carries four level tables t (S, C) -- gains of y and of z and their inverses -- and codes at a quality q
in [0, S-1] held as float32.  The gain-vector rule, per table and channel c:
    s = min(int(floorf(q)), S - 2),  f = q - s,
    a = fma(f, t[s+1][c], fmul(1 - f, t[s][c]))             (float32: 1 - f and the lower level's product rounded
                                                             once each, the upper level's product fused with the sum)
    g[c] = 1.0f if a == 0 else expf(a)
so an integer q gives exp(t[q]), the values between interpolate geometrically, and zero tables give gains of
exactly 1.0.  With (g_y, g_y', g_z, g_z') the four vectors at q, every product one float32 multiplication per
element: the symbols of z are rint(z * g_z); h_s reads z_hat = rint(z * g_z) * g_z'; the symbols of y are
rint(y * g_y - mu); the reconstruction handed to g_s is (q_y + mu) * g_y'.  Tables, rows, chunks and payloads are
those of the mean-scale streams (conditional kind 2 or 3).  Both sides compute the gain vectors on the device, by
the same kernel (csrc/gain.hip), from the float32 quality the stream stores: the decoder never takes it from the
model.
    "ICRG" (batch):     the "ICRA" header with this magic, format version 1, then u32 S, f32 quality,
                        then the chunk lengths and payloads as in "ICRA";
    "ICRQ" (per image): the "ICRP" header with this magic, format version 1, then u32 S, f32 quality (this image's:
                        the images of a call may differ), then the chunk lengths and payloads as in "ICRP".
S >= 2 and a finite quality in [0, S-1], or the parser raises ValueError; a model with another S refuses the stream.
The six containers do not read one another: every parser raises ValueError on another's magic.

Region containers (little endian): `RegionGainedMeanScaleCompressor2018`, a quality per 64 x 64 pixel block
------------------------------------------------------------------------------------------------------------
A quality map is uint8 codes k[n, bi, bj], one per 64 x 64 block of the padded image: bi < H/64, bj < W/64.  The
quality of a code, for a model with S levels, is
    q(k) = fdiv(float32(k * (S - 1)), 255.0f)             (one correctly rounded float32 division of two exact integers)
so q(0) = 0 and q(255) = S - 1 exactly, q is monotone in k, and an integer level s is a code exactly when
255 % (S - 1) == 0 (the default S = 6: k = 51 s).  Position (i, j) of y belongs to block (i >> 2, j >> 2), position
(i, j) of z is block (i, j).  Both sides obtain the gains in the same way:
    1. U = the distinct codes of the call (of the group of streams decoded together), ascending;
    2. the gain-vector rule above at the qualities [q(u) for u in U], by the same kernel: R = len(U) <= 256 rows per
       table;
    3. every position takes the row whose index is the rank of its block's code in U.
A row is a function of its code alone, so the gains of an image do not depend on what else is coded or decoded with
it, and a uniform map of code k holds bit for bit the gains of the gained model at quality q(k).  The symbols, h_s,
the tables, rows, chunks and payloads are those of the gained streams with the gain vectors taken per position.
    "ICRM" (batch):     the "ICRA" header with this magic, format version 1, then u32 S, u32 map_h, u32 map_w,
                        then N * map_h * map_w code bytes in (n, bi, bj) order,
                        then the chunk lengths and payloads as in "ICRA";
    "ICRR" (per image): the "ICRP" header with this magic, format version 1, then u32 S, u32 map_h, u32 map_w,
                        then map_h * map_w code bytes in (bi, bj) order (this image's map),
                        then the chunk lengths and payloads as in "ICRP".
The conditional kind is 2 or 3.  S >= 2, map_h == H/64 and map_w == W/64, and the buffer holds the whole map, or the
parser raises ValueError; a model with another S refuses the stream.  The decoder takes the map from the stream.
The eight containers do not read one another: every parser raises ValueError on another's magic.

Coding to a byte budget (`GainedMeanScaleCompressor2018.compress_each_to`): the search rule
--------------------------------------------------------------------------------------------
A budget B is a bound on len() of one image's "ICRQ" stream, header included.  The size of a candidate quality is
measured, never estimated: `image_stream_bytes` of the chunk lengths the coder itself reports for that candidate.
Sizes are not assumed monotone in the quality (the gain tables are learnt), so the search is a grid search in
`rounds` rounds of `candidates` = Q qualities, per image:
    round 1 searches `budget_grid(S, Q)`: float32(k (S-1) / (Q-1)), k = 0 .. Q-1, the quotient in float64;
    a round's choice is `budget_choice`: the largest of its candidates whose size is <= B (the largest that fits,
        not the one before the first that fails);
    every later round searches `budget_refine(chosen, next, Q)`: float32(lo + j (hi - lo) / (Q+1)), j = 1 .. Q, in
        float64, of which only the values strictly inside (lo, hi) are kept, once each, ascending; `next` is
        `budget_next`: the next larger quality among everything measured for the image so far.  `chosen` stays when
        none of them fits;
    an image whose choice is S-1 has no later round; nor has one for which no candidate of round 1 fits: that is a
        `BudgetError` (strict), or the image is coded at quality 0 and is the one stream that may exceed its budget.
The result is optimal relative to the qualities measured, not to the interval.

A quality map under a byte budget (`RegionGainedMeanScaleCompressor2018.compress_each_map_to`): the allocation rule
--------------------------------------------------------------------------------------------------------------------
A budget B is a bound on len() of one image's "ICRR" stream, header and map included.  The map is chosen block by
block at one slope t in [0, S-1] per image, and t is searched by the rule above; the budget is enforced on sizes the
coder itself reports, so it is exact, while the tables that steer the choice are an estimate.
    Levels.  The S integer levels q_l = l, l = 0 .. S-1; the code of level l is `map_level_codes(S)[l]` =
        quality_code(l, S) and its gains are those of code_quality(code_l, S), as the uniform map of set_quality(l).
    Tables.  bits[n, l, b] and sse[n, l, b], float32, (N, S, Hb Wb): bit for bit the `bits` and `sse` that
        `rate_distortion_map(x)` returns on the same batch after set_quality(l).  g_a and h_a do not depend on the
        quality and run once for the S levels.
    Allocation at slope t (`map_allocate`).  w = `map_weight(loss_weight(t), x.shape[1])` = float32(lambda(t) / C), the
        weight of `compress_each_refined`'s J = B + w D.  For every block b, J[l] = fadd(bits[l, b], fmul(w, sse[l, b])),
        each operation rounded once in float32, none contracted.  l is scanned 0 .. S-1 ascending from best = 0 and
        replaces best iff J[l] < J[best] (strict): a tie goes to the lower level, a NaN never wins.  The map holds
        code_best(b).  It is the exact minimiser of the tabulated sum of J over independent per-block choices and
        nothing more: neighbouring blocks share receptive fields, so the table is a steering estimate.
    Search over t.  The search rule above, unchanged: round 1 is `budget_grid(S, Q)`, later rounds `budget_refine`,
        with `budget_choice` and `budget_next`; sizes are not assumed monotone in t.  A miss is a `BudgetError`
        (strict), or the image is coded with the map of round 1's first slope (t = 0) and is the one stream that may
        exceed its budget.
    Size of a candidate.  `image_stream_bytes(region_image_fixed_bytes(header), lz, ly)` from the chunk lengths the
        coder reports; the map travels raw in the header, so the fixed part does not depend on the map.
The streams are ordinary "ICRR" streams: byte for byte what `set_quality_map(map)` followed by `compress_each` writes.

Encode-time latent refinement (`Compressor2018.compress_each_refined`): the rule
---------------------------------------------------------------------------------
The decoder's inputs stay fixed: the weights and the hyper-latent, and so (sigma, mu).  Only the integers of y change,
so the streams are ordinary "ICRP" / "ICRQ" streams and `decompress_each` reads them as it reads any other.  For a
call on N images, `_pad_each` and `_analyse(x, each=True)` give y, the symbols of z and kz (coded as `compress_each`
codes them, never touched) and (sigma, mu) as the decoder will compute them.  The loop works in the coded domain,
v0 = `_latent_gain(y)`; mu absent means that no subtraction and no addition is performed.
    Evaluate(v):  s = symbol_of(v - mu) (one fp32 subtraction, the symbolizers' rule); y_hat = float(s) + mu (one fp32
        addition); x_hat = `_reconstruct(_latent_ungain(y_hat))` on the padded batch; D_n = the sum of (x - x_hat)^2
        over the padded image n; B_n = the sum over image n of the rate term clamp(-log2(p + 1e-10), 0, 50) of p, the
        conditional likelihood of y_hat under (sigma, mu) (the kernel `conditional_likelihood` runs);
        J_n = B_n + w_n D_n in fp64 with w_n = lambda_n / x.shape[1], image n's share of the training loss times its
        pixel count; lambda_n is `distortion_loss_weight`, on the gained model `loss_weight(q_n)` of that image's
        quality.
    Gradient:  g = d(sum_n w_n D_n) / d y_hat + d(sum of the rate terms of p(v | sigma, mu)) / dv: the first term through
        the clamp and g_s, passed straight through the rounding to v; the second the likelihood at the unrounded v.
    Update:  Adam on v, moments m = u = 0 at the start, beta1 = 0.9, beta2 = 0.999, eps = 1e-8, the bias corrections
        1 / (1 - beta^t) formed on the host in double and passed as fp32; every fp32 operation rounded once, in the
        order csrc/refine.hip states.
    Keep-best:  T + 1 evaluations, evaluation 0 the unrefined latent, whose symbols are bit for bit `compress_each`'s.
        The symbols of evaluation t replace image n's kept symbols iff J_n(t) < best_n: strict, a NaN never wins, every
        image decides alone.  After the last evaluation the kept symbols are coded: their per-image kmax first (the
        same refusal above 2047 as `compress_each`), then `encode_symbols_seg` and `_pack_image`.
So J_after <= J_before for every image, always, and steps = 0 gives `compress_each`'s bytes.

Decoding a pixel window of a per-image stream (`Compressor2018.decompress_window`): the plan
-------------------------------------------------------------------------------------------
The formats above are unchanged; a window decode reads less of an "ICRP" / "ICRQ" / "ICRR" stream.  `window_plan(header,
box, kernel, strides)` says what it reads, for the box (top, left, height, width) in pixels of the unpadded h x w image;
a box that is empty or leaves [0, h) x [0, w) is a ValueError in front of everything else.
    Latent window (`latent_window`).  Start from the pixel intervals [top, top + height - 1] and [left, left + width - 1]
        and walk g_s's layers backwards: a transposed conv with kernel k, stride s and padding k // 2 maps the output
        interval [a, b] to the input interval [ceil((a + k // 2 - (k - 1)) / s), floor((b + k // 2) / s)], clipped to
        that level's extent after every layer (the extent of the level in front of a layer is the one behind it over s;
        the last one is the padded latent).  For kernel 5 and strides [2, 2, 2, 2] that is at most 2 latent positions
        beyond the box on each side.  The result is snapped outward to multiples of MAP_BLOCK // Y_DOWN = 4 latent
        positions and clipped to the padded latent: rows [r0, r1), columns [c0, c1), whole 64 x 64 blocks of the padded
        image, the grid of the quality maps.  GDN is pointwise, so g_s on that window alone gives, at
        crop = (top - D r0, left - D c0) with D the product of the strides (16), the pixels of the box up to the
        arithmetic's rounding.
    Symbols and chunks.  y's symbols are in (h, w, c) order, so rows [r0, r1) are the symbols [r0 Wy C, r1 Wy C) and
        those lie in the chunks [k0, k1) = [r0 Wy C // (64 R), ceil(r1 Wy C / (64 R))), each decodable alone; their bytes
        follow from the length table.  A chunk is decoded whole (a lane's states are serial); a symbol is kept where its
        (row, column) lies in the window.
    What is read whole.  z is small and decoded whole; h_s runs on the whole z at batch shape 1, because its sigma bits
        select the table rows (the rule of the per-image container); the rows and the mean of the window are taken from
        the whole sigma and mu.
    `byte_ranges` (with the streams' chunk-length tables given): the (begin, end) ranges of the stream a window decode
        reads, ascending and disjoint: the header with its variable-length section, both length tables and z's payload,
        then y's chunks k0 .. k1 - 1.  Nothing else of the stream influences the result.
The decoded window of y_hat holds bit for bit the values `decompress_each` holds there.

Transcoding in the latent domain (`Compressor2018.transcode_each`, `GainedMeanScaleCompressor2018.transcode_each_to`)
---------------------------------------------------------------------------------------------------------------------
A per-image stream ("ICRP" / "ICRQ" / "ICRR") becomes another stream of the same model without passing through pixels:
neither g_a nor g_s runs.  The formats above are unchanged.
    Re-chunking.  The symbols of z and of y are decoded and coded again at another R = steps_per_chunk; y is decoded
        without its mean (the residual integers), under the rows of sigma = h_s(z_hat) evaluated once.  The output's
        header is the parsed one with R replaced (`transcoded_header`): kmax_z, kmax_y, the quality and the map stay.
        The result is bit for bit the stream `compress_each` writes for the same image at that R.
    Requantization ("ICRQ" only).  From the stream's quality q1 to a quality q2 != q1; the gain vectors
        (g_y, g_y', g_z, g_z') at q1 and at q2 are the gain-vector rule's, from the stored float32 values.  Every *, +, -
        below is one float32 operation, rounded once, never contracted with another; (sigma, mu) = h_s(.) is evaluated
        on one stream at a time (batch shape 1), as everywhere in the per-image streams:
            k_z1 = the decoded integers of z          z_hat1 = k_z1 * g_z'(q1)       (sigma1, mu1) = h_s(z_hat1)
            k_z2 = symbol_of(z_hat1 * g_z(q2))        z_hat2 = k_z2 * g_z'(q2)       (sigma2, mu2) = h_s(z_hat2)
            r1   = the decoded integers of y (the residual about mu1)
            k_y2 = symbol_of(((r1 + mu1) * g_y'(q1)) * g_y(q2) - mu2)
        (r1 + mu1) * g_y'(q1) is exactly the y_hat that g_s would read.  y is coded with the rows of sigma2 and the tables
        of its own K; the header is the parsed one with quality = q2 and kmax_z, kmax_y, R replaced.  A symbol beyond
        KMAX_LIMIT is a ValueError naming the stream.  At q2 == q1 nothing is requantized (the stream is returned, or
        only re-chunked): g' * g is not 1 for learnt tables, so an equal quality must not cost a generation.
    To a byte budget (`transcode_each_to`).  A stream is first re-chunked where another R is asked; one that then
        holds at most its budget is the result, at its own quality q1.  Otherwise the search rule of
        `compress_each_to` above runs on the sizes the coder reports for the requantized candidates, with two
        differences:
            round 1 searches `transcode_grid(S, Q, q1)` = [q for q in budget_grid(S, Q) if q < q1]: transcoding upwards
                buys bytes and no quality.  An empty list (q1 = 0) is a miss, as is a round 1 of which nothing fits;
            what is measured for the stream starts as `transcode_measured(q1, len(stream))` = {q1: len(stream)}, so that
                `budget_next` / `budget_refine` refine between the top grid point below q1 and q1, strictly inside.
        A miss is a `BudgetError` (strict) in front of the packing of any requantized stream -- for a stream at q1 = 0
        that already has the target R, in front of any launch; one that has to be re-chunked is judged at its
        re-chunked length, which may fit -- or the stream at quality 0 (for q1 = 0 the stream itself, re-chunked where
        asked): the one result that may exceed its budget.

Layered per-image containers (`Compressor2018.compress_each_layered` / `decompress_each_layered`)
-------------------------------------------------------------------------------------------------
A per-image stream whose every byte prefix that holds the tables decodes to an image: y is coded in channel layers, and
a layer that has not arrived reconstructs as the hyperprior's own prediction.
    Layers.  y has C channels; they form G layers, 1 <= G <= C, C % G == 0, Cg = C // G.  Each image has a channel
        order o, a permutation of 0 .. C-1; layer g holds the channels o[g Cg .. (g + 1) Cg - 1], and its symbols are
        those channels' symbols in (h, w, j) order, j the place inside the layer, fastest.  The symbols are the
        unchanged ones of `compress_each`: rint(y), rint(y - mu), or on the gained model rint(y * g_y - mu).  Each
        layer is a bitstream of its own exactly as "Bitstream of one tensor" specifies, its chunks cut from the layer's
        first symbol; the row of each symbol is index(sigma) at its own (position, channel).  One kmax_y per image
        serves all layers -- the largest |symbol| of the image, as in "ICRP" -- and so one table.
    Default order (`layer_order(energy)`).  The channels by descending energy[c] = the sum over positions of symbol^2,
        an exact integer; ties go to the lower channel index.  Over the layers dropped, this sum is the coded-domain
        squared error a decoder incurs by putting mu in their place.  It is a steering rule only, and a heuristic: the
        decoder reads the order from the stream.  order="identity" and an explicit (C,) or (N, C) integer array are
        accepted (`layer_orders`); anything that is not a permutation is a ValueError before any launch.
    Absent layers.  A decoder that holds the layers 0 .. L-1 (0 <= L <= G) reconstructs the coded-domain latent as
        q + mu on their channels -- ic_add_mean's one fp32 addition -- and on all other channels as mu, bit for bit, or
        +0.0 where the model has no mean.  Then `_latent_ungain` and g_s run as always.  L = 0 is the hyperprior's own
        picture of the image.
    Containers.  "ICRL" is the "ICRP" header and "ICRH" the "ICRQ" header (u32 S, f32 quality where "ICRQ" has
        them), with the field "chunks of y" replaced by "chunks of one layer" (every layer has nsym_y / G symbols and
        so the same chunk count) and u32 G appended to the fixed header.  After the fixed header: C x u16, the channel
        order (the variable-length section); then the chunk lengths of z, the chunk lengths of the layers 0 .. G-1, the
        payload of z, the payloads of the layers 0 .. G-1.  All tables lie in front of all payloads, so any prefix that
        holds the tables says where every layer ends.  Format version 1, or INVARIANT_FORMAT_VERSION for the h_s
        route, as in every other per-image container; each route refuses the other's streams.
    Prefixes.  `layer_ends(data)` = G + 1 byte offsets from the header and the tables alone: ends[0] the end of z's
        payload, ends[g] the end of layer g-1.  `parse_layered_image(..., prefix=True)` accepts any buffer of at least
        ends[0] bytes and returns the whole layers it holds, L = max{g : ends[g] <= len(data)}; the bytes of a partly
        arrived layer are ignored.  Without `prefix` the length must be ends[G] exactly.
    Refusals (ValueError, before any launch): a buffer that ends inside the header, the order table or the length
        tables; one shorter than ends[0]; G outside 1 .. C; C % G != 0; an order that is not a permutation; a chunk
        length that fails the checks of every container.
The existing parsers refuse the two magics and the two parsers refuse the existing ones: the ten containers do not read
one another.
"""
import dataclasses
import math
import struct
from dataclasses import dataclass

import numpy as np

MAGIC = b"ICRA"
FORMAT_VERSION = 1
INVARIANT_FORMAT_VERSION = 2   # h_s by the batch-invariant kernel: every container but "ICRC" (3 and 4 there)
KMAX_LIMIT = 2047          # IC_CODEC_KMAX: 2K+1 <= 4095 counts of >= 1 inside a 16-bit total
MAX_SCALES = 256           # IC_CODEC_MAXL: rows are uint8
MAX_STEPS = 65536          # IC_CODEC_MAXR
KIND_MEAN = 2              # bit 1 of the conditional kind: y coded about a mean from h_s
PRECISION = 16
CHUNK_HEAD = 256           # 64 lanes x 4 bytes of state
COMPUTE_DTYPES = ("fp32_split", "fp32", "bf16")
Y_DOWN, Z_DOWN = 16, 64    # image pixels per latent / hyper-latent sample, each way

_FIELDS = "<4sHBBIIIIIIIddIIIQQ"   # what every container's header starts with: magic .. symbols of y; chunk counts follow
_HEAD = struct.Struct(_FIELDS + "II")

IMAGE_MAGIC = b"ICRP"
IMAGE_FORMAT_VERSION = 1
_IMAGE_HEAD = struct.Struct(_FIELDS + "II" + "II")   # the ICRA header's fields, then image height and width

CKBD_MAGIC = b"ICRC"
CKBD_FORMAT_VERSION = 1          # the context from the two convs
CKBD_FUSED_FORMAT_VERSION = 2    # the context from the fused, batch-invariant kernel
CKBD_INVARIANT_FORMAT_VERSION = 3         # the two above with h_s by the batch-invariant kernel
CKBD_FUSED_INVARIANT_FORMAT_VERSION = 4
_CKBD_HEAD = struct.Struct(_FIELDS + "III")   # the ICRA header's fields with three chunk counts: z, y anchors, y non-anchors
CKBD_IMAGE_MAGIC = b"ICRK"
CKBD_IMAGE_FORMAT_VERSION = 1
_CKBD_IMAGE_HEAD = struct.Struct(_FIELDS + "III" + "II")   # the ICRC header, then image height and width

GAINED_MAGIC = b"ICRG"
GAINED_IMAGE_MAGIC = b"ICRQ"
GAINED_FORMAT_VERSION = 1
_GAINED_HEAD = struct.Struct(_FIELDS + "II" + "If")               # the ICRA header, then the gain levels and the quality
_GAINED_IMAGE_HEAD = struct.Struct(_FIELDS + "II" + "II" + "If")  # the ICRP header, then the same two

REGION_MAGIC = b"ICRM"
REGION_IMAGE_MAGIC = b"ICRR"
REGION_FORMAT_VERSION = 1
MAP_BLOCK = Z_DOWN         # a quality-map block is 64 x 64 pixels: one position of z, 4 x 4 of y
MAP_CODE_MAX = 255
_REGION_HEAD = struct.Struct(_FIELDS + "II" + "III")               # the ICRA header, then the gain levels and the map's shape
_REGION_IMAGE_HEAD = struct.Struct(_FIELDS + "II" + "II" + "III")  # the ICRP header, then the same three


@dataclass
class Header:
    N: int
    H: int
    W: int
    latent_channels: int
    hyper_channels: int
    kind: int
    compute_dtype: str
    abi: int
    L: int
    scale_min: float
    scale_max: float
    R: int
    kmax_z: int
    kmax_y: int

    @property
    def z_shape(self):
        return (self.N, self.hyper_channels, self.H // Z_DOWN, self.W // Z_DOWN)

    @property
    def y_shape(self):
        return (self.N, self.latent_channels, self.H // Y_DOWN, self.W // Y_DOWN)

    @property
    def nsym_z(self):
        return int(np.prod(self.z_shape, dtype=np.int64))

    @property
    def nsym_y(self):
        return int(np.prod(self.y_shape, dtype=np.int64))


@dataclass
class ImageHeader(Header):
    """Header of the per-image container: N = 1, H x W the padded size, height x width the image's."""
    height: int
    width: int


@dataclass
class GainedHeader(Header):
    """Header of the gained batch container: the model's number of gain levels S and the quality the batch was
    coded at, a float32 value in [0, S-1]."""
    levels: int
    quality: float


@dataclass
class GainedImageHeader(ImageHeader):
    """Header of the gained per-image container: ImageHeader, then the levels and this image's quality."""
    levels: int
    quality: float


class _MapEq:
    """Equality of the region headers: field by field, the code maps as arrays."""
    _array_field = "codes"

    def __eq__(self, other):
        if type(other) is not type(self):
            return NotImplemented
        a, b = dict(vars(self)), dict(vars(other))
        ca, cb = a.pop(self._array_field), b.pop(self._array_field)
        return a == b and (ca is cb or (ca is not None and cb is not None and np.array_equal(ca, cb)))

    __hash__ = None


@dataclass(eq=False)
class RegionHeader(_MapEq, Header):
    """Header of the region batch container: the model's number of gain levels S, the shape of the quality map and
    its codes, uint8 (N, map_h, map_w)."""
    levels: int
    map_h: int
    map_w: int
    codes: np.ndarray = None


@dataclass(eq=False)
class RegionImageHeader(_MapEq, ImageHeader):
    """Header of the region per-image container: ImageHeader, then the levels, the map's shape and this image's codes,
    uint8 (map_h, map_w)."""
    levels: int
    map_h: int
    map_w: int
    codes: np.ndarray = None


class _OrderEq(_MapEq):
    """Equality of the layered headers: field by field, the channel orders as arrays."""
    _array_field = "order"


@dataclass(eq=False)
class LayeredImageHeader(_OrderEq, ImageHeader):
    """Header of the layered per-image container: ImageHeader, then the number of layers G and this image's channel
    order, int32 (latent_channels,)."""
    layers: int
    order: np.ndarray = None


@dataclass(eq=False)
class LayeredGainedImageHeader(_OrderEq, GainedImageHeader):
    """Header of the layered gained per-image container: GainedImageHeader, then the layers and the order."""
    layers: int
    order: np.ndarray = None


def padded_size(h, w):
    """(H, W): h and w rounded up to multiples of 64, the size that is coded."""
    return -(-int(h) // Z_DOWN) * Z_DOWN, -(-int(w) // Z_DOWN) * Z_DOWN


def num_chunks(nsym, R):
    return -(-int(nsym) // (64 * int(R)))


def scale_table(L, scale_min, scale_max):
    """(scales float32[L], midpoints float32[L-1]) of the log-spaced scale table, from float64."""
    lo, hi = math.log(float(scale_min)), math.log(float(scale_max))
    s = [math.exp(lo + t * (hi - lo) / (L - 1)) for t in range(L)] if L > 1 else [float(scale_min)]
    mids = [math.sqrt(s[t] * s[t + 1]) for t in range(L - 1)]
    return np.asarray(s, dtype=np.float32), np.asarray(mids, dtype=np.float32)


def _check_header(h):
    if h.compute_dtype not in COMPUTE_DTYPES:
        raise ValueError(f"codec: unknown COMPUTE_DTYPE {h.compute_dtype!r}")
    if h.kind not in (0, 1, 2, 3):
        raise ValueError(f"codec: unknown conditional kind {h.kind}")
    if min(h.N, h.H, h.W, h.latent_channels, h.hyper_channels) < 1:
        raise ValueError("codec: empty batch shape")
    if h.H % Z_DOWN or h.W % Z_DOWN:
        raise ValueError(f"codec: image size {h.H}x{h.W} is not a multiple of {Z_DOWN}")
    if not 1 <= h.L <= MAX_SCALES:
        raise ValueError(f"codec: {h.L} scales (1..{MAX_SCALES})")
    if not (math.isfinite(h.scale_min) and math.isfinite(h.scale_max) and 0.0 < h.scale_min
            and (h.scale_min < h.scale_max or h.L == 1)):
        raise ValueError(f"codec: bad scale range [{h.scale_min}, {h.scale_max}]")
    if not 1 <= h.R <= MAX_STEPS:
        raise ValueError(f"codec: steps_per_chunk {h.R} (1..{MAX_STEPS})")
    for name, k in (("kmax_z", h.kmax_z), ("kmax_y", h.kmax_y)):
        if not 0 <= k <= KMAX_LIMIT:
            raise ValueError(f"codec: {name} = {k} exceeds the coder's limit of {KMAX_LIMIT}")


def _check_lengths(name, lens, nsym, R):
    if len(lens) != num_chunks(nsym, R):
        raise ValueError(f"codec: {len(lens)} {name} chunk lengths for {nsym} symbols at R = {R}")
    per = 64 * R
    for c, n in enumerate(lens.tolist()):
        words = min(per, nsym - c * per)
        if n < CHUNK_HEAD or n % 2 or n > CHUNK_HEAD + 2 * words:
            raise ValueError(f"codec: {name} chunk {c} of {words} symbols cannot be {n} bytes long")


# ---- the framing all three containers share: header, one chunk-length table per stream, one payload per stream.
# The first stream is z; the streams of y are named by `y_names` and hold `y_symbols(h)` symbols.
def _whole_y(h):
    return (h.nsym_y,)


def _fixed_bytes(head, h, y_symbols=_whole_y, var=0):
    nc = sum(num_chunks(n, h.R) for n in (h.nsym_z, *y_symbols(h)))
    return head.size + var + 4 * nc + CHUNK_HEAD * nc


def _route_version(version, conv):
    """`version` of a container whose conv-route number is `conv`: that, or INVARIANT_FORMAT_VERSION."""
    if version not in (conv, INVARIANT_FORMAT_VERSION):
        raise ValueError(f"codec: no format version {version} of this container ({conv}: h_s through the conv plans, "
                         f"{INVARIANT_FORMAT_VERSION}: h_s by the batch-invariant kernel)")
    return int(version)


def _pack(head, magic, version, check, h, lens, payloads, extra=(), y_names=("y",), y_symbols=_whole_y, var=b""):
    """One bytes object from the header `h`, which `check` passes, the streams' chunk-length tables and their
    payloads; `extra`: the header fields after the chunk counts; `var`: the bytes of the header's variable-length
    section, between the fixed header and the tables."""
    check(h)
    lens = [np.ascontiguousarray(l, dtype="<u4") for l in lens]
    payloads = [bytes(p) for p in payloads]
    for name, l, nsym in zip(("z", *y_names), lens, (h.nsym_z, *y_symbols(h))):
        _check_lengths(name, l, nsym, h.R)
    if any(int(l.sum(dtype=np.uint64)) != len(p) for l, p in zip(lens, payloads)):
        raise ValueError("codec: chunk lengths do not add up to the payload")
    fields = (COMPUTE_DTYPES.index(h.compute_dtype), h.kind, h.abi, h.N, h.H, h.W, h.latent_channels, h.hyper_channels,
              h.L, h.scale_min, h.scale_max, h.R, h.kmax_z, h.kmax_y, h.nsym_z, h.nsym_y, *map(len, lens), *extra)
    return b"".join([head.pack(magic, version, *fields), bytes(var)] + [l.tobytes() for l in lens] + payloads)


def _parse_header(data, abi, compute_dtype, head, magic, versions, header, check, k):
    """(checked header object, the k chunk counts, symbols of z, symbols of y) of the fixed header `head` at the start
    of `data`: the magic, the version (one of `versions`), the arithmetic tag and the ABI against the running build
    (`abi` None: a reader that decodes nothing checks neither), then `header(common fields, fields after the chunk
    counts)` passed through `check`."""
    if len(data) < head.size:
        raise ValueError(f"codec: {len(data)} bytes is shorter than the header ({head.size})")
    (s_magic, ver, dt, kind, s_abi, N, H, W, cy, cz, L, smin, smax, R, kz, ky, nz, ny,
     *rest) = head.unpack_from(data, 0)
    counts, extra = rest[:k], rest[k:]
    if s_magic != magic:
        raise ValueError(f"codec: bad magic {s_magic!r}")
    if ver not in versions:
        raise ValueError(f"codec: format version {ver}, this build reads {' or '.join(map(str, versions))}")
    if dt >= len(COMPUTE_DTYPES):
        raise ValueError(f"codec: unknown arithmetic tag {dt}")
    if abi is not None:
        if COMPUTE_DTYPES[dt] != compute_dtype:
            raise ValueError(f"codec: stream coded with COMPUTE_DTYPE {COMPUTE_DTYPES[dt]!r}, the model runs "
                             f"{compute_dtype!r}")
        if s_abi != abi:
            raise ValueError(f"codec: stream coded by library ABI {s_abi}, this build is {abi}")
    h = header(N, H, W, cy, cz, kind, COMPUTE_DTYPES[dt], s_abi, L, smin, smax, R, kz, ky, *extra)
    check(h)
    return h, counts, nz, ny


def _parse(data, abi, compute_dtype, head, magic, version, header, check, y_names=("y",), y_symbols=_whole_y, note="",
           var=None):
    """(header, the streams' chunk-length tables, their payloads) of a container: the header `head` with its magic
    and version, the header object `header(common fields, fields after the chunk counts)` passed through `check`,
    and every check of the counts, the tables and the payload.  `note` ends the message about the symbol counts.
    `var` = (size, take): the header has a variable-length section of `size(h)` bytes after its fixed part, which
    `take(h, bytes)` stores in the checked header."""
    data = bytes(data)
    k = 1 + len(y_names)
    h, counts, nz, ny = _parse_header(data, abi, compute_dtype, head, magic, (version,), header, check, k)
    R = h.R
    nsyms = (h.nsym_z, *y_symbols(h))
    if nz != nsyms[0] or any(len(y_names) * n != ny for n in nsyms[1:]):   # the streams of y hold equal shares of it
        raise ValueError(f"codec: symbol counts do not match the batch shape{note}")
    if any(c != num_chunks(n, R) for c, n in zip(counts, nsyms)):
        raise ValueError("codec: chunk counts do not match the symbol counts")
    off = head.size
    if var is not None:
        size, take = var
        if len(data) < off + size(h):
            raise ValueError(f"codec: buffer ends inside the header's variable-length section of {size(h)} bytes")
        take(h, data[off:off + size(h)])
        off += size(h)
    if len(data) < off + 4 * sum(counts):
        raise ValueError("codec: buffer ends inside the chunk-length tables")
    tables = []
    for name, c, n in zip(("z", *y_names), counts, nsyms):
        tables.append(np.frombuffer(data, dtype="<u4", count=c, offset=off))
        off += 4 * c
        _check_lengths(name, tables[-1], n, R)
    sizes = [int(t.sum(dtype=np.uint64)) for t in tables]
    if off + sum(sizes) != len(data):
        raise ValueError(f"codec: chunk lengths add up to {sum(sizes)} payload bytes, the buffer holds {len(data) - off}")
    ends = [off + sum(sizes[:i]) for i in range(k + 1)]
    return (h, *tables, *(data[a:b] for a, b in zip(ends, ends[1:])))


def fixed_bytes(h):
    """The bytes of a container that do not depend on the symbols: header, length tables and the
    256 bytes of lane states per chunk."""
    return _fixed_bytes(_HEAD, h)


def pack(h, lens_z, lens_y, payload_z, payload_y, version=FORMAT_VERSION):
    """One bytes object from the header, the two chunk-length tables and the two payloads."""
    v = _route_version(version, FORMAT_VERSION)
    return _pack(_HEAD, MAGIC, v, _check_header, h, (lens_z, lens_y), (payload_z, payload_y))


def parse(data, abi, compute_dtype, version=FORMAT_VERSION):
    """(Header, lens_z, lens_y, payload_z, payload_y) of a container made by `pack`; `abi` and
    `compute_dtype` are the running build's ic_version() and the model's arithmetic, which the
    stream must match.  Raises ValueError on anything inconsistent; nothing is launched here."""
    v = _route_version(version, FORMAT_VERSION)
    return _parse(data, abi, compute_dtype, _HEAD, MAGIC, v, Header, _check_header)


def _check_image_header(h):
    _check_header(h)
    if h.N != 1:
        raise ValueError(f"codec: a per-image stream holds one image, not {h.N}")
    for name, full, part in (("height", h.H, h.height), ("width", h.W, h.width)):
        if not 1 <= part <= full or full - part >= Z_DOWN:
            raise ValueError(f"codec: image {name} {part} does not pad to {full}")


def image_fixed_bytes(h):
    """`fixed_bytes` of a per-image container."""
    return _fixed_bytes(_IMAGE_HEAD, h)


def pack_image(h, lens_z, lens_y, payload_z, payload_y, version=IMAGE_FORMAT_VERSION):
    """One bytes object for one image from its ImageHeader, chunk-length tables and payloads."""
    v = _route_version(version, IMAGE_FORMAT_VERSION)
    return _pack(_IMAGE_HEAD, IMAGE_MAGIC, v, _check_image_header, h, (lens_z, lens_y), (payload_z, payload_y),
                 (h.height, h.width))


def parse_image(data, abi, compute_dtype, version=IMAGE_FORMAT_VERSION):
    """(ImageHeader, lens_z, lens_y, payload_z, payload_y) of a container made by `pack_image`: the
    checks of `parse`, and those of the image size.  Nothing is launched here."""
    v = _route_version(version, IMAGE_FORMAT_VERSION)
    return _parse(data, abi, compute_dtype, _IMAGE_HEAD, IMAGE_MAGIC, v, ImageHeader, _check_image_header)


# ---- checkerboard container "ICRC": y in two bitstreams, the anchors and the non-anchors
def checkerboard_count(h, w, parity):
    """Positions (i, j) with (i + j) % 2 == parity in one h x w map (ic_ckbd_count)."""
    if h < 1 or w < 1 or parity not in (0, 1):
        raise ValueError(f"codec: no checkerboard half {parity} of a {h} x {w} map")
    return (h * w + 1 - parity) // 2


def checkerboard_order(h, w, parity):
    """The flat positions i * w + j of one map's half `parity`, in the order the half is packed (ascending): entry
    k by the rule of the gather / scatter kernels -- two consecutive rows hold w positions of a parity between
    them, `first` of them in the even row."""
    first = (w - parity + 1) // 2
    k = np.arange(checkerboard_count(h, w, parity), dtype=np.int64)
    pair, rem = k // w, k % w
    odd = rem >= first
    i = 2 * pair + odd
    j = np.where(odd, (1 - parity) + 2 * (rem - first), parity + 2 * rem)
    return i * w + j


def _check_checkerboard_header(h):
    _check_header(h)
    if not h.kind & KIND_MEAN:
        raise ValueError(f"codec: conditional kind {h.kind} in a checkerboard stream, which codes y about a mean (2 or 3)")


def _half_symbols(h):
    """(symbols of the anchor half, of the non-anchor half) of y."""
    _, C, hh, ww = h.y_shape
    return tuple(h.N * C * checkerboard_count(hh, ww, p) for p in (0, 1))


_HALVES = ("y anchor", "y non-anchor")


def checkerboard_fixed_bytes(h):
    """`fixed_bytes` of a checkerboard container: three streams, each half of y chunked on its own."""
    return _fixed_bytes(_CKBD_HEAD, h, _half_symbols)


def checkerboard_version(version, invariant=False):
    """The number on the wire: `version` (1 or 2) names the route of the context, `invariant` that of h_s."""
    if version not in (CKBD_FORMAT_VERSION, CKBD_FUSED_FORMAT_VERSION):
        raise ValueError(f"codec: no checkerboard format version {version}")
    return int(version) + (CKBD_INVARIANT_FORMAT_VERSION - CKBD_FORMAT_VERSION if invariant else 0)


def pack_checkerboard(h, lens_z, lens_ya, lens_yn, payload_z, payload_ya, payload_yn, version=CKBD_FORMAT_VERSION,
                      invariant=False):
    """One bytes object from the header, the three chunk-length tables and the three payloads (z, the anchors
    of y, the non-anchors of y); `version`: 1 -- the context came from the convs, 2 -- from the fused kernel.
    `invariant`: h_s ran through the batch-invariant kernel; the container then carries 3 or 4 in their place."""
    return _pack(_CKBD_HEAD, CKBD_MAGIC, checkerboard_version(version, invariant), _check_checkerboard_header, h,
                 (lens_z, lens_ya, lens_yn), (payload_z, payload_ya, payload_yn), (), _HALVES, _half_symbols)


def parse_checkerboard(data, abi, compute_dtype, version=CKBD_FORMAT_VERSION, invariant=False):
    """(Header, lens_z, lens_ya, lens_yn, payload_z, payload_ya, payload_yn) of a container made by
    `pack_checkerboard` with this `version` and `invariant`, with the checks of `parse`.  Raises ValueError on anything
    inconsistent, every other version included; nothing is launched here."""
    return _parse(data, abi, compute_dtype, _CKBD_HEAD, CKBD_MAGIC, checkerboard_version(version, invariant), Header,
                  _check_checkerboard_header, _HALVES, _half_symbols, " (y in two equal halves)")


# ---- per-image checkerboard container "ICRK": one image of a "fused" checkerboard model
def _check_checkerboard_image_header(h):
    _check_image_header(h)
    _check_checkerboard_header(h)


def checkerboard_image_fixed_bytes(h):
    """`fixed_bytes` of a per-image checkerboard container."""
    return _fixed_bytes(_CKBD_IMAGE_HEAD, h, _half_symbols)


def pack_checkerboard_image(h, lens_z, lens_ya, lens_yn, payload_z, payload_ya, payload_yn,
                            version=CKBD_IMAGE_FORMAT_VERSION):
    """One bytes object for one image from its ImageHeader, the three chunk-length tables and the three payloads."""
    v = _route_version(version, CKBD_IMAGE_FORMAT_VERSION)
    return _pack(_CKBD_IMAGE_HEAD, CKBD_IMAGE_MAGIC, v, _check_checkerboard_image_header, h,
                 (lens_z, lens_ya, lens_yn), (payload_z, payload_ya, payload_yn), (h.height, h.width), _HALVES,
                 _half_symbols)


def parse_checkerboard_image(data, abi, compute_dtype, version=CKBD_IMAGE_FORMAT_VERSION):
    """(ImageHeader, lens_z, lens_ya, lens_yn, payload_z, payload_ya, payload_yn) of a container made by
    `pack_checkerboard_image`: the checks of `parse_checkerboard`, and those of the image size.  Nothing is
    launched here."""
    v = _route_version(version, CKBD_IMAGE_FORMAT_VERSION)
    return _parse(data, abi, compute_dtype, _CKBD_IMAGE_HEAD, CKBD_IMAGE_MAGIC, v, ImageHeader,
                  _check_checkerboard_image_header, _HALVES, _half_symbols, " (y in two equal halves)")


# ---- gained containers "ICRG" (batch) and "ICRQ" (per image): the mean-scale streams of a model with gain units
def _check_gain(h):
    if h.levels < 2:
        raise ValueError(f"codec: {h.levels} gain levels (at least 2)")
    if not (math.isfinite(h.quality) and 0.0 <= h.quality <= h.levels - 1):
        raise ValueError(f"codec: quality {h.quality} is outside [0, {h.levels - 1}]")
    if h.quality != float(np.float32(h.quality)):
        raise ValueError(f"codec: quality {h.quality!r} is not a float32 value")


def _check_gained_header(h):
    _check_header(h)
    _check_gain(h)


def _check_gained_image_header(h):
    _check_image_header(h)
    _check_gain(h)


def gained_fixed_bytes(h):
    """`fixed_bytes` of a gained batch container."""
    return _fixed_bytes(_GAINED_HEAD, h)


def gained_image_fixed_bytes(h):
    """`fixed_bytes` of a gained per-image container."""
    return _fixed_bytes(_GAINED_IMAGE_HEAD, h)


def pack_gained(h, lens_z, lens_y, payload_z, payload_y, version=GAINED_FORMAT_VERSION):
    """One bytes object from a GainedHeader, the two chunk-length tables and the two payloads."""
    v = _route_version(version, GAINED_FORMAT_VERSION)
    return _pack(_GAINED_HEAD, GAINED_MAGIC, v, _check_gained_header, h, (lens_z, lens_y), (payload_z, payload_y),
                 (h.levels, h.quality))


def parse_gained(data, abi, compute_dtype, version=GAINED_FORMAT_VERSION):
    """(GainedHeader, lens_z, lens_y, payload_z, payload_y) of a container made by `pack_gained`: the checks of
    `parse`, and those of the levels and the quality.  Nothing is launched here."""
    v = _route_version(version, GAINED_FORMAT_VERSION)
    return _parse(data, abi, compute_dtype, _GAINED_HEAD, GAINED_MAGIC, v, GainedHeader, _check_gained_header)


def pack_gained_image(h, lens_z, lens_y, payload_z, payload_y, version=GAINED_FORMAT_VERSION):
    """One bytes object for one image from its GainedImageHeader, chunk-length tables and payloads."""
    v = _route_version(version, GAINED_FORMAT_VERSION)
    return _pack(_GAINED_IMAGE_HEAD, GAINED_IMAGE_MAGIC, v, _check_gained_image_header, h, (lens_z, lens_y),
                 (payload_z, payload_y), (h.height, h.width, h.levels, h.quality))


def parse_gained_image(data, abi, compute_dtype, version=GAINED_FORMAT_VERSION):
    """(GainedImageHeader, lens_z, lens_y, payload_z, payload_y) of a container made by `pack_gained_image`: the
    checks of `parse_image`, and those of the levels and the quality.  Nothing is launched here."""
    v = _route_version(version, GAINED_FORMAT_VERSION)
    return _parse(data, abi, compute_dtype, _GAINED_IMAGE_HEAD, GAINED_IMAGE_MAGIC, v, GainedImageHeader,
                  _check_gained_image_header)


# ---- layered per-image containers "ICRL" and "ICRH": y in G channel layers, any prefix that holds the tables decodes
LAYERED_IMAGE_MAGIC = b"ICRL"
LAYERED_GAINED_IMAGE_MAGIC = b"ICRH"
LAYERED_FORMAT_VERSION = 1
_LAYERED_IMAGE_HEAD = struct.Struct(_FIELDS + "II" + "II" + "I")          # the ICRP header, then the layers
_LAYERED_GAINED_IMAGE_HEAD = struct.Struct(_FIELDS + "II" + "II" + "If" + "I")   # the ICRQ header, then the layers
MAX_LAYER_CHANNELS = 65535     # the order table holds u16 channel numbers


def layer_order(energy):
    """The default channel order from energy (C,) or (N, C), non-negative integers (the sum over positions of
    symbol^2): the channels by descending energy, ties to the lower channel index; int32, the shape of `energy`."""
    e = np.asarray(energy)
    if e.dtype.kind not in "iu" or e.ndim not in (1, 2) or e.shape[-1] < 1 or (e.size and e.min() < 0):
        raise ValueError(f"codec: the energies are non-negative integers (C,) or (N, C), got {e.dtype} {e.shape}")
    if e.size and int(e.max()) > np.iinfo(np.int64).max:
        raise ValueError("codec: an energy beyond 2^63")
    return np.argsort(-e.astype(np.int64), axis=-1, kind="stable").astype(np.int32)


def _check_order(order, C):
    o = np.asarray(order)
    if o.dtype.kind not in "iu" or o.shape != (C,) or not np.array_equal(np.sort(o.astype(np.int64)), np.arange(C)):
        raise ValueError(f"codec: a channel order is a permutation of 0 .. {C - 1}")


def layer_orders(order, N, C):
    """int32 (N, C): the channel order of every image of a call from `order` = "identity", a (C,) array for all of
    them or an (N, C) array.  ValueError for anything that is not a permutation of 0 .. C-1 per image."""
    if isinstance(order, str):
        if order != "identity":
            raise ValueError(f"codec: order is 'energy', 'identity' or an integer array, got {order!r}")
        return np.tile(np.arange(C, dtype=np.int32), (N, 1))
    o = np.asarray(order)
    if o.dtype.kind not in "iu" or o.shape not in ((C,), (N, C)):
        raise ValueError(f"codec: an explicit order is an integer array ({C},) or ({N}, {C}), got {o.dtype} {o.shape}")
    o = np.broadcast_to(o, (N, C))
    for row in o:
        _check_order(row, C)
    return np.ascontiguousarray(o, dtype=np.int32)


def _check_layers(h):
    C, G = h.latent_channels, h.layers
    if C > MAX_LAYER_CHANNELS:
        raise ValueError(f"codec: a layered stream numbers at most {MAX_LAYER_CHANNELS} channels, got {C}")
    if isinstance(G, bool) or int(G) != G or not 1 <= G <= C:
        raise ValueError(f"codec: {G} layers of {C} channels (1 .. {C})")
    if C % G:
        raise ValueError(f"codec: {G} layers do not divide {C} channels")
    if h.order is not None:
        _check_order(h.order, C)


def _check_layered_image_header(h):
    _check_image_header(h)
    _check_layers(h)


def _check_layered_gained_image_header(h):
    _check_gained_image_header(h)
    _check_layers(h)


# (fixed header, magic, header class, its check, the header fields after the chunk counts) of the two containers
_LAYERED = {
    False: (_LAYERED_IMAGE_HEAD, LAYERED_IMAGE_MAGIC, LayeredImageHeader, _check_layered_image_header,
            lambda h: (h.height, h.width, h.layers)),
    True: (_LAYERED_GAINED_IMAGE_HEAD, LAYERED_GAINED_IMAGE_MAGIC, LayeredGainedImageHeader,
           _check_layered_gained_image_header, lambda h: (h.height, h.width, h.levels, h.quality, h.layers)),
}


def _layer_symbols(h):
    return h.nsym_y // h.layers


def layered_image_fixed_bytes(h):
    """`fixed_bytes` of a layered per-image container (either kind, by the header's type), the order table included."""
    head = _LAYERED[isinstance(h, LayeredGainedImageHeader)][0]
    nc = num_chunks(h.nsym_z, h.R) + h.layers * num_chunks(_layer_symbols(h), h.R)
    return head.size + 2 * h.latent_channels + 4 * nc + CHUNK_HEAD * nc


def _pack_layered(gained, h, lens_z, lens_layers, payload_z, payload_layers, version):
    head, magic, cls, check, extra = _LAYERED[gained]
    v = _route_version(version, LAYERED_FORMAT_VERSION)
    if type(h) is not cls:
        raise ValueError(f"codec: this container takes a {cls.__name__}, not a {type(h).__name__}")
    check(h)
    if h.order is None:
        raise ValueError("codec: a layered header without its channel order")
    lens = [np.ascontiguousarray(l, dtype="<u4") for l in (lens_z, *lens_layers)]
    payloads = [bytes(p) for p in (payload_z, *payload_layers)]
    if len(lens) != h.layers + 1 or len(payloads) != h.layers + 1:
        raise ValueError(f"codec: {len(lens) - 1} length tables and {len(payloads) - 1} payloads for {h.layers} layers")
    _check_lengths("z", lens[0], h.nsym_z, h.R)
    for g, l in enumerate(lens[1:]):
        _check_lengths(f"y layer {g}", l, _layer_symbols(h), h.R)
    if any(int(l.sum(dtype=np.uint64)) != len(p) for l, p in zip(lens, payloads)):
        raise ValueError("codec: chunk lengths do not add up to the payload")
    fields = (COMPUTE_DTYPES.index(h.compute_dtype), h.kind, h.abi, h.N, h.H, h.W, h.latent_channels, h.hyper_channels,
              h.L, h.scale_min, h.scale_max, h.R, h.kmax_z, h.kmax_y, h.nsym_z, h.nsym_y, len(lens[0]), len(lens[1]),
              *extra(h))
    order = np.ascontiguousarray(h.order, dtype="<u2").tobytes()
    return b"".join([head.pack(magic, v, *fields), order] + [l.tobytes() for l in lens] + payloads)


def _layered_layout(data, gained, abi, compute_dtype, versions):
    """(header, [the length table of z, of layer 0, ..], [ends[0], .., ends[G]]) of a layered container or of a prefix
    of one that holds the header, the order table and the length tables; nothing behind the tables is read."""
    head, magic, cls, check, _ = _LAYERED[gained]
    h, counts, nz, ny = _parse_header(data, abi, compute_dtype, head, magic, versions, cls, check, 2)
    if nz != h.nsym_z or ny != h.nsym_y:
        raise ValueError("codec: symbol counts do not match the image shape")
    nsyms = (h.nsym_z, _layer_symbols(h))
    if any(c != num_chunks(n, h.R) for c, n in zip(counts, nsyms)):
        raise ValueError("codec: chunk counts do not match the symbol counts")
    off, C, G = head.size, h.latent_channels, h.layers
    if len(data) < off + 2 * C:
        raise ValueError(f"codec: buffer ends inside the channel order of {2 * C} bytes")
    order = np.frombuffer(data, dtype="<u2", count=C, offset=off).astype(np.int32)
    _check_order(order, C)
    h.order = order
    off += 2 * C
    if len(data) < off + 4 * (counts[0] + G * counts[1]):
        raise ValueError("codec: buffer ends inside the chunk-length tables")
    tables = []
    for g in range(G + 1):
        c = counts[min(g, 1)]
        tables.append(np.frombuffer(data, dtype="<u4", count=c, offset=off))
        off += 4 * c
        _check_lengths("z" if g == 0 else f"y layer {g - 1}", tables[-1], nsyms[min(g, 1)], h.R)
    ends = (off + np.cumsum([int(t.sum(dtype=np.uint64)) for t in tables], dtype=np.int64)).tolist()
    return h, tables, [off, *ends]


def _parse_layered(data, gained, abi, compute_dtype, version, prefix):
    v = _route_version(version, LAYERED_FORMAT_VERSION)
    data = bytes(data)
    h, tables, (first, *ends) = _layered_layout(data, gained, abi, compute_dtype, (v,))
    if prefix:
        if len(data) < ends[0]:
            raise ValueError(f"codec: a prefix of {len(data)} bytes ends in front of the end of z's payload at {ends[0]}")
        held = max(g for g in range(h.layers + 1) if ends[g] <= len(data))
    else:
        if len(data) != ends[-1]:
            raise ValueError(f"codec: the tables put the stream's end at {ends[-1]} bytes, the buffer holds {len(data)}")
        held = h.layers
    return (h, tables[0], tables[1:], data[first:ends[0]], [data[ends[g]:ends[g + 1]] for g in range(held)])


def pack_layered_image(h, lens_z, lens_layers, payload_z, payload_layers, version=LAYERED_FORMAT_VERSION):
    """One bytes object for one image from its LayeredImageHeader, the length table of z, those of the G layers, the
    payload of z and those of the G layers."""
    return _pack_layered(False, h, lens_z, lens_layers, payload_z, payload_layers, version)


def parse_layered_image(data, abi, compute_dtype, version=LAYERED_FORMAT_VERSION, prefix=False):
    """(LayeredImageHeader, lens_z, [lens of layer g for all G], payload_z, [payload of layer g for the L layers held])
    of a container made by `pack_layered_image`.  Without `prefix` the buffer is the whole stream and L = G; with it,
    any prefix of at least `layer_ends(data)[0]` bytes, L the whole layers it holds.  Nothing is launched here."""
    return _parse_layered(data, False, abi, compute_dtype, version, prefix)


def pack_layered_gained_image(h, lens_z, lens_layers, payload_z, payload_layers, version=LAYERED_FORMAT_VERSION):
    """`pack_layered_image` for a LayeredGainedImageHeader."""
    return _pack_layered(True, h, lens_z, lens_layers, payload_z, payload_layers, version)


def parse_layered_gained_image(data, abi, compute_dtype, version=LAYERED_FORMAT_VERSION, prefix=False):
    """`parse_layered_image` for a container made by `pack_layered_gained_image`: the checks of the levels and the
    quality besides."""
    return _parse_layered(data, True, abi, compute_dtype, version, prefix)


def layer_ends(data):
    """[ends[0], .., ends[G]] of a layered stream ("ICRL" or "ICRH", either format version) or of any prefix of it that
    holds the header, the order table and the length tables: ends[0] is the end of z's payload and ends[g] the end of
    layer g-1, in bytes from the stream's start.  The build that decodes is not consulted: nothing is decoded here."""
    data = bytes(data)
    magics = {LAYERED_IMAGE_MAGIC: False, LAYERED_GAINED_IMAGE_MAGIC: True}
    if data[:4] not in magics:
        raise ValueError(f"codec: bad magic {data[:4]!r}")
    versions = (LAYERED_FORMAT_VERSION, INVARIANT_FORMAT_VERSION)
    return _layered_layout(data, magics[data[:4]], None, None, versions)[2][1:]


# ---- coding to a byte budget: the search rule of `compress_each_to` (the docstring's last section)
class BudgetError(ValueError):
    """No candidate of the first round fits an image's budget: `image` (its index in the call), `budget` (bytes)
    and `smallest` (the smallest stream measured for it, bytes)."""

    def __init__(self, image, budget, smallest):
        super().__init__(f"codec: image {image} does not fit {budget} bytes at any quality searched: its smallest "
                         f"stream is {smallest} bytes")
        self.image, self.budget, self.smallest = int(image), int(budget), int(smallest)


def _check_candidates(Q, least):
    if isinstance(Q, bool) or not isinstance(Q, (int, np.integer)) or Q < least:
        raise ValueError(f"codec: the number of candidates is an integer >= {least}, got {Q!r}")
    return int(Q)


def budget_grid(S, Q):
    """The Q >= 2 qualities of round 1 for a model with S levels, ascending: 0 and S-1 exactly at the ends."""
    S, Q = _check_levels(S), _check_candidates(Q, 2)
    return [float(np.float32(k * (S - 1) / (Q - 1))) for k in range(Q)]


def budget_refine(lo, hi, Q):
    """Up to Q qualities strictly inside (lo, hi), ascending and distinct: the float32 values of lo + j (hi - lo) /
    (Q + 1), j = 1 .. Q, that are neither end.  Empty when no float32 lies between the two."""
    Q, lo, hi = _check_candidates(Q, 1), float(lo), float(hi)
    if not lo <= hi:     # NaN included
        raise ValueError(f"codec: no interval ({lo!r}, {hi!r}) to refine")
    qs = {float(np.float32(lo + j * (hi - lo) / (Q + 1))) for j in range(1, Q + 1)}
    return sorted(q for q in qs if lo < q < hi)


def budget_choice(qualities, sizes, budget):
    """The largest of `qualities` whose entry of `sizes` is <= budget, or None when none is."""
    fit = [q for q, n in zip(qualities, sizes) if n <= budget]
    return max(fit) if fit else None


def budget_next(measured, chosen):
    """The next larger quality than `chosen` among `measured`, or None."""
    above = [q for q in measured if q > chosen]
    return min(above) if above else None


def transcode_grid(S, Q, q1):
    """Round 1 of `transcode_each_to` for a stream coded at quality q1: the qualities of `budget_grid(S, Q)` strictly
    below q1, ascending.  Empty at q1 = 0."""
    q1 = float(q1)
    if not 0.0 <= q1 <= _check_levels(S) - 1:    # NaN included
        raise ValueError(f"codec: quality {q1!r} is outside [0, {S - 1}]")
    return [q for q in budget_grid(S, Q) if q < q1]


def transcode_measured(q1, size):
    """What is measured for a stream of `size` bytes coded at quality q1 before `transcode_each_to` measures anything:
    the stream itself, the upper end of every later refinement."""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1:
        raise ValueError(f"codec: a stream's size is a positive int, a number of bytes, got {size!r}")
    return {float(q1): int(size)}


def transcoded_header(h, **changes):
    """The header of a transcoded per-image stream: the parsed header `h` with `changes` among R, quality, kmax_z and
    kmax_y replaced; everything else, a region stream's map included, is the parsed stream's."""
    if not isinstance(h, ImageHeader):
        raise ValueError(f"codec: a per-image stream's header is transcoded, not a {type(h).__name__}")
    allowed = {"R", "kmax_z", "kmax_y"} | ({"quality"} if isinstance(h, GainedImageHeader) else set())
    if not set(changes) <= allowed:
        raise ValueError(f"codec: transcoding a {type(h).__name__} replaces {sorted(allowed)}, not "
                         f"{sorted(set(changes) - allowed)}")
    return dataclasses.replace(h, **changes)


def image_stream_bytes(fixed, *lens):
    """len() of a per-image stream whose `*_image_fixed_bytes` is `fixed` and whose chunk-length tables are `lens`:
    the fixed part counts every chunk's 256 bytes of lane states, the lengths count them again."""
    return int(fixed) + sum(int(np.asarray(l, dtype=np.int64).sum()) - CHUNK_HEAD * len(l) for l in lens)


# ---- a quality map under a byte budget: the allocation rule of `compress_each_map_to` (the docstring's section)
MAP_MAX_LEVELS = 16        # the levels one allocation chooses among (ic_block_allocate)


def map_level_codes(S):
    """The codes of the S integer levels, [quality_code(l, S) for l = 0 .. S-1]: what a map chosen by the allocation
    rule holds."""
    return [quality_code(l, S) for l in range(_check_levels(S))]


def map_weight(lam, channels):
    """float32(lam / channels) as a Python float: the weight w of J = B + w D for a distortion weight `lam` (the
    model's `loss_weight(t)`) and an image of `channels` channels."""
    if isinstance(channels, bool) or int(channels) != channels or channels < 1:
        raise ValueError(f"codec: an image has at least 1 channel, got {channels!r}")
    w = float(np.float32(float(lam) / int(channels)))
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError(f"codec: the weight of an allocation is finite and >= 0, got {lam!r} / {channels!r}")
    return w


def map_allocate(bits, sse, w):
    """The level of every block at the weight w: bits, sse (L, nb) float32 tables -> (nb,) uint8, by the allocation
    rule: J[l] = fadd(bits[l], fmul(w, sse[l])) in float32, l scanned ascending from best = 0 and replacing best iff
    J[l] < J[best] (strict: a tie keeps the lower level, a NaN never wins)."""
    bits, sse = np.asarray(bits), np.asarray(sse)
    if bits.dtype != np.float32 or sse.dtype != np.float32 or bits.ndim != 2 or bits.shape != sse.shape:
        raise ValueError(f"codec: the tables are float32 (levels, blocks) arrays of one shape, got {bits.dtype} "
                         f"{bits.shape} and {sse.dtype} {sse.shape}")
    if not 2 <= bits.shape[0] <= MAP_MAX_LEVELS or bits.shape[1] < 1:
        raise ValueError(f"codec: an allocation chooses among 2 .. {MAP_MAX_LEVELS} levels for at least 1 block, got "
                         f"{bits.shape}")
    w = np.float32(w)
    if not (np.isfinite(w) and w >= 0):
        raise ValueError(f"codec: the weight of an allocation is finite and >= 0, got {w!r}")
    with np.errstate(all="ignore"):
        J = bits + w * sse                   # one float32 product, then one float32 sum, per element
    best, best_j = np.zeros(bits.shape[1], dtype=np.uint8), J[0].copy()
    for l in range(1, bits.shape[0]):
        take = J[l] < best_j
        best[take], best_j[take] = l, J[l][take]
    return best


# ---- region containers "ICRM" (batch) and "ICRR" (per image): the gained streams with a quality per 64 x 64 block
def _check_levels(S):
    if isinstance(S, bool) or int(S) != S or S < 2:
        raise ValueError(f"codec: {S} gain levels (at least 2)")
    return int(S)


def code_quality(k, S):
    """The float32 quality of the code k (0 .. 255) for a model with S levels, as a Python float: one correctly
    rounded float32 division of k * (S - 1) by 255.  An array of codes gives a float32 array."""
    S = _check_levels(S)
    a = np.asarray(k)
    if a.dtype.kind not in "iu" or a.size and (a.min() < 0 or a.max() > MAP_CODE_MAX):
        raise ValueError(f"codec: a quality code is an integer in [0, {MAP_CODE_MAX}], got {k!r}")
    q = (a.astype(np.int64) * (S - 1)).astype(np.float32) / np.float32(MAP_CODE_MAX)
    return float(q) if a.ndim == 0 else q


def quality_code(q, S):
    """The code nearest to the quality q in [0, S-1]: rint(q * 255 / (S - 1)), ties to even.  ValueError outside the
    range, NaN included."""
    S = _check_levels(S)
    try:
        v = float("nan") if isinstance(q, (bool, str, bytes)) else float(q)
    except (TypeError, ValueError):
        raise ValueError(f"codec: a quality is a number in [0, {S - 1}], got {q!r}") from None
    if not 0.0 <= v <= S - 1:    # NaN fails both comparisons
        raise ValueError(f"codec: quality {q!r} is outside [0, {S - 1}]")
    return int(np.rint(v * MAP_CODE_MAX / (S - 1)))


def block_map(h, w, S, background, regions=()):
    """The code map (ceil(h / 64), ceil(w / 64)), uint8, of an h x w image: `background` everywhere, and for every
    (top, left, height, width, quality) pixel rectangle of `regions` each block it touches raised to the rectangle's
    code -- a block takes the largest quality that touches it, the background's included.  ValueError for a
    rectangle that is empty or leaves the image."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"codec: no quality map of a {h} x {w} image")
    codes = np.full((-(-h // MAP_BLOCK), -(-w // MAP_BLOCK)), quality_code(background, S), dtype=np.uint8)
    for top, left, height, width, quality in regions:
        top, left, height, width = int(top), int(left), int(height), int(width)
        if height < 1 or width < 1 or top < 0 or left < 0 or top + height > h or left + width > w:
            raise ValueError(f"codec: rectangle {(top, left, height, width)} is empty or leaves the {h} x {w} image")
        blk = codes[top // MAP_BLOCK:(top + height - 1) // MAP_BLOCK + 1, left // MAP_BLOCK:(left + width - 1) // MAP_BLOCK + 1]
        np.maximum(blk, np.uint8(quality_code(quality, S)), out=blk)
    return codes


def _check_map(h, shape):
    if h.levels < 2:
        raise ValueError(f"codec: {h.levels} gain levels (at least 2)")
    if (h.map_h, h.map_w) != (h.H // MAP_BLOCK, h.W // MAP_BLOCK):
        raise ValueError(f"codec: a {h.map_h} x {h.map_w} quality map for a {h.H} x {h.W} image, which has "
                         f"{h.H // MAP_BLOCK} x {h.W // MAP_BLOCK} blocks")
    if not h.kind & KIND_MEAN:
        raise ValueError(f"codec: conditional kind {h.kind} in a region stream, which codes y about a mean (2 or 3)")
    if h.codes is not None and (not isinstance(h.codes, np.ndarray) or h.codes.dtype != np.uint8 or h.codes.shape != shape):
        raise ValueError(f"codec: the quality map must be uint8 codes of shape {shape}")


def _check_region_header(h):
    _check_header(h)
    _check_map(h, (h.N, h.map_h, h.map_w))


def _check_region_image_header(h):
    _check_image_header(h)
    _check_map(h, (h.map_h, h.map_w))


def _map_bytes(h):
    return h.N * h.map_h * h.map_w


def _take_map(image):
    def take(h, data):
        h.codes = np.frombuffer(data, dtype=np.uint8).reshape((h.map_h, h.map_w) if image else (h.N, h.map_h, h.map_w))
    return take


def _packed_map(h):
    if h.codes is None:
        raise ValueError("codec: a region header without its quality map")
    return np.ascontiguousarray(h.codes).tobytes()


def region_fixed_bytes(h):
    """`fixed_bytes` of a region batch container, the code map included."""
    return _fixed_bytes(_REGION_HEAD, h, var=_map_bytes(h))


def region_image_fixed_bytes(h):
    """`fixed_bytes` of a region per-image container, the code map included."""
    return _fixed_bytes(_REGION_IMAGE_HEAD, h, var=_map_bytes(h))


def pack_region(h, lens_z, lens_y, payload_z, payload_y, version=REGION_FORMAT_VERSION):
    """One bytes object from a RegionHeader, the two chunk-length tables and the two payloads."""
    _check_region_header(h)
    v = _route_version(version, REGION_FORMAT_VERSION)
    return _pack(_REGION_HEAD, REGION_MAGIC, v, _check_region_header, h, (lens_z, lens_y), (payload_z, payload_y),
                 (h.levels, h.map_h, h.map_w), var=_packed_map(h))


def parse_region(data, abi, compute_dtype, version=REGION_FORMAT_VERSION):
    """(RegionHeader, lens_z, lens_y, payload_z, payload_y) of a container made by `pack_region`: the checks of
    `parse`, and those of the levels and the map.  Nothing is launched here."""
    v = _route_version(version, REGION_FORMAT_VERSION)
    return _parse(data, abi, compute_dtype, _REGION_HEAD, REGION_MAGIC, v, RegionHeader, _check_region_header,
                  var=(_map_bytes, _take_map(False)))


def pack_region_image(h, lens_z, lens_y, payload_z, payload_y, version=REGION_FORMAT_VERSION):
    """One bytes object for one image from its RegionImageHeader, chunk-length tables and payloads."""
    _check_region_image_header(h)
    v = _route_version(version, REGION_FORMAT_VERSION)
    return _pack(_REGION_IMAGE_HEAD, REGION_IMAGE_MAGIC, v, _check_region_image_header, h, (lens_z, lens_y),
                 (payload_z, payload_y), (h.height, h.width, h.levels, h.map_h, h.map_w), var=_packed_map(h))


def parse_region_image(data, abi, compute_dtype, version=REGION_FORMAT_VERSION):
    """(RegionImageHeader, lens_z, lens_y, payload_z, payload_y) of a container made by `pack_region_image`: the
    checks of `parse_image`, and those of the levels and the map.  Nothing is launched here."""
    v = _route_version(version, REGION_FORMAT_VERSION)
    return _parse(data, abi, compute_dtype, _REGION_IMAGE_HEAD, REGION_IMAGE_MAGIC, v, RegionImageHeader,
                  _check_region_image_header, var=(_map_bytes, _take_map(True)))


# ---- decoding a pixel window of a per-image stream: what it reads (the docstring's last section)
LATENT_SNAP = MAP_BLOCK // Y_DOWN   # a latent window is whole map blocks: multiples of 4 latent positions


@dataclass(frozen=True)
class WindowPlan:
    """What a window decode of one per-image stream reads and where the box lies in what g_s returns for it."""
    box: tuple           # (top, left, height, width), pixels of the unpadded image
    rows: tuple          # (r0, r1): latent rows [r0, r1)
    cols: tuple          # (c0, c1): latent columns [c0, c1)
    crop: tuple          # (top - D r0, left - D c0): the box's corner in g_s of the latent window
    symbols: tuple       # (r0 Wy C, r1 Wy C): the range of y's symbols that holds the rows
    chunks: tuple        # (k0, k1): the chunks of y, at the header's R, that hold those symbols
    byte_ranges: tuple   # ((begin, end), ...) of the stream, or None when no length tables were given

    @property
    def shape(self):
        """(rh, rw) of the latent window."""
        return self.rows[1] - self.rows[0], self.cols[1] - self.cols[0]


def _walk_back(a, b, extent, kernel, strides):
    """The closed latent interval that the pixels [a, b] of g_s's output depend on; `extent`: the latent's."""
    down = math.prod(strides)
    for s in reversed(strides):
        down //= s
        p = kernel // 2
        a, b = -((kernel - 1 - p - a) // s), (b + p) // s     # ceil((a + p - (k - 1)) / s), floor((b + p) / s)
        a, b = max(a, 0), min(b, extent * down - 1)
    return a, b


def latent_window(box, latent_hw, kernel, strides):
    """(r0, r1, c0, c1, (crop_top, crop_left)) of the pixel box (top, left, height, width) of g_s's output for a
    latent of `latent_hw` = (Hy, Wy) positions: the walk, the snap to LATENT_SNAP and the clip of the docstring.
    g_s is len(strides) transposed convs of `kernel` x `kernel` taps, padding kernel // 2, with pointwise layers
    between them.  ValueError for a box that is empty or leaves the output."""
    kernel, strides = int(kernel), [int(s) for s in strides]
    if kernel < 1 or not strides or min(strides) < 1:
        raise ValueError(f"codec: no synthesis transform with kernel {kernel} and strides {strides}")
    top, left, height, width = (int(v) for v in box)
    D = math.prod(strides)
    Hy, Wy = (int(v) for v in latent_hw)
    if height < 1 or width < 1 or top < 0 or left < 0 or top + height > D * Hy or left + width > D * Wy:
        raise ValueError(f"codec: box {(top, left, height, width)} is empty or leaves the {D * Hy} x {D * Wy} output")
    out = []
    for a, n, extent in ((top, height, Hy), (left, width, Wy)):
        lo, hi = _walk_back(a, a + n - 1, extent, kernel, strides)
        out += [lo // LATENT_SNAP * LATENT_SNAP, min(-(-(hi + 1) // LATENT_SNAP) * LATENT_SNAP, extent)]
    return (*out, (top - D * out[0], left - D * out[2]))


def _image_head_bytes(h):
    """The bytes in front of the length tables of the per-image container that `h` is the header of."""
    if isinstance(h, RegionImageHeader):
        return _REGION_IMAGE_HEAD.size + _map_bytes(h)
    if isinstance(h, GainedImageHeader):
        return _GAINED_IMAGE_HEAD.size
    if isinstance(h, ImageHeader):
        return _IMAGE_HEAD.size
    raise ValueError(f"codec: a window is planned on a per-image stream's header, not on a {type(h).__name__}")


def window_plan(header, box, kernel, strides, lengths=None):
    """The WindowPlan of the pixel box (top, left, height, width) of the stream whose parsed per-image header is
    `header` ("ICRP", "ICRQ" or "ICRR"), for a g_s of MODEL.CONV_KERNEL `kernel` and MODEL.STRIDES `strides`.
    `lengths` = (chunk lengths of z, of y) as the parser returns them: with them `byte_ranges` is filled in.
    ValueError, in front of everything else, for a box that is empty or leaves [0, h) x [0, w)."""
    try:
        top, left, height, width = (int(v) for v in box)
    except (TypeError, ValueError):
        raise ValueError(f"codec: a box is (top, left, height, width), got {box!r}") from None
    if not isinstance(header, ImageHeader):
        raise ValueError(f"codec: a window is planned on a per-image stream's header, not on a {type(header).__name__}")
    if height < 1 or width < 1 or top < 0 or left < 0 or top + height > header.height or left + width > header.width:
        raise ValueError(f"codec: box {(top, left, height, width)} is empty or leaves the {header.height} x "
                         f"{header.width} image")
    if math.prod(int(s) for s in strides) != Y_DOWN:
        raise ValueError(f"codec: strides {list(strides)} do not make the streams' {Y_DOWN} pixels per latent position")
    _, C, Hy, Wy = header.y_shape
    r0, r1, c0, c1, crop = latent_window((top, left, height, width), (Hy, Wy), kernel, strides)
    s0, s1 = r0 * Wy * C, r1 * Wy * C
    per = 64 * header.R
    k0, k1 = s0 // per, -(-s1 // per)
    ranges = None
    if lengths is not None:
        lens_z, lens_y = (np.asarray(l, dtype=np.int64) for l in lengths)
        if len(lens_z) != num_chunks(header.nsym_z, header.R) or len(lens_y) != num_chunks(header.nsym_y, header.R):
            raise ValueError("codec: the chunk-length tables are not the header's")
        y_at = _image_head_bytes(header) + 4 * (len(lens_z) + len(lens_y)) + int(lens_z.sum())
        ends = np.concatenate(([0], np.cumsum(lens_y)))
        begin, end = y_at + int(ends[k0]), y_at + int(ends[k1])
        ranges = ((0, end),) if begin == y_at else ((0, y_at), (begin, end))
    return WindowPlan((top, left, height, width), (r0, r1), (c0, c1), crop, (s0, s1), (k0, k1), ranges)


def split_packed_seg(packed, nseg, seg_len, R):
    """[(lengths, payload bytes)] per segment of the segmented coder's output buffer
    [all lengths][all payload][padding]: stream s is found by summing the lengths before it."""
    packed = np.asarray(packed, dtype=np.uint8)
    cps = num_chunks(seg_len, R)
    lens = packed[:4 * cps * nseg].view("<u4").copy().reshape(nseg, cps)
    ends = np.cumsum(lens.sum(axis=1, dtype=np.uint64))
    if 4 * cps * nseg + int(ends[-1]) > packed.size:
        raise RuntimeError("codec: the coder reported more bytes than its buffer holds")
    body = packed[4 * cps * nseg:]
    return [(lens[s], body[int(ends[s - 1]) if s else 0:int(ends[s])].tobytes()) for s in range(nseg)]


def join_packed_seg(parts):
    """The segmented decoder's input [all lengths][all payload] from [(lengths, payload)] per segment."""
    lens = b"".join(np.ascontiguousarray(l, dtype="<u4").tobytes() for l, _ in parts)
    return np.frombuffer(lens + b"".join(bytes(p) for _, p in parts), dtype=np.uint8)


def split_packed(packed, nsym, R):
    """(lengths, payload bytes) of the device coder's output buffer [lengths][payload][padding]."""
    return split_packed_seg(packed, 1, nsym, R)[0]


def join_packed(lens, payload):
    """The device decoder's input buffer [lengths][payload] as a uint8 array."""
    return np.frombuffer(np.ascontiguousarray(lens, dtype="<u4").tobytes() + bytes(payload), dtype=np.uint8)
