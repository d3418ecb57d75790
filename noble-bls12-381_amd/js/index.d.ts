// Type declarations of the facade (index.js): the exported surface of paulmillr/noble-bls12-381 v1.4.0 (index.ts:22, 715-821)
// plus the additive batched entry points of the MI355X engine.
export type Hex = Uint8Array | string;
export type PrivateKey = Hex | bigint | number;

export declare const CURVE: {
  P: bigint; r: bigint; h: bigint; Gx: bigint; Gy: bigint; b: bigint; P2: bigint; h2: bigint;
  G2x: [bigint, bigint]; G2y: [bigint, bigint]; b2: [bigint, bigint]; x: bigint; h2Eff: bigint;
};

interface Field<T> {
  isZero(): boolean; equals(rhs: T): boolean; negate(): T; add(rhs: T): T; subtract(rhs: T): T; invert(): T;
  multiply(rhs: T | bigint): T; square(): T; pow(n: bigint): T; div(rhs: T | bigint): T;
}
export declare class Fp implements Field<Fp> {
  static readonly ORDER: bigint; static readonly MAX_BITS: number; static readonly BYTES_LEN: number; static readonly ZERO: Fp; static readonly ONE: Fp;
  readonly value: bigint;
  constructor(value: bigint);
  isZero(): boolean; equals(rhs: Fp): boolean; negate(): Fp; invert(): Fp; add(rhs: Fp): Fp; subtract(rhs: Fp): Fp; square(): Fp;
  multiply(rhs: Fp | bigint): Fp; div(rhs: Fp | bigint): Fp; pow(n: bigint): Fp; sqrt(): Fp | undefined; toString(): string;
  static fromBytes(b: Uint8Array): Fp; toBytes(): Uint8Array;
}
export declare class Fr implements Field<Fr> {
  static readonly ORDER: bigint; static readonly ZERO: Fr; static readonly ONE: Fr; static isValid(b: bigint): boolean;
  readonly value: bigint;
  constructor(value: bigint);
  isZero(): boolean; equals(rhs: Fr): boolean; negate(): Fr; invert(): Fr; add(rhs: Fr): Fr; subtract(rhs: Fr): Fr; square(): Fr;
  multiply(rhs: Fr | bigint): Fr; div(rhs: Fr | bigint): Fr; pow(n: bigint): Fr; legendre(): Fr; sqrt(): Fr | undefined; toString(): string;
}
export declare class Fp2 implements Field<Fp2> {
  static readonly ORDER: bigint; static readonly MAX_BITS: number; static readonly BYTES_LEN: number; static readonly ZERO: Fp2; static readonly ONE: Fp2;
  readonly c0: Fp; readonly c1: Fp;
  constructor(c0: Fp, c1: Fp);
  static fromBigTuple(t: [bigint, bigint] | bigint[]): Fp2;
  one(): Fp2; isZero(): boolean; equals(rhs: Fp2): boolean; reim(): { re: bigint; im: bigint }; negate(): Fp2; add(rhs: Fp2): Fp2; subtract(rhs: Fp2): Fp2;
  multiply(rhs: Fp2 | bigint): Fp2; square(): Fp2; pow(n: bigint): Fp2; div(rhs: Fp2 | bigint): Fp2; invert(): Fp2; sqrt(): Fp2 | undefined;
  mulByNonresidue(): Fp2; multiplyByB(): Fp2; frobeniusMap(power: number): Fp2; toString(): string;
  static fromBytes(b: Uint8Array): Fp2; toBytes(): Uint8Array;
}
export declare class Fp6 implements Field<Fp6> {
  static readonly BYTES_LEN: number; static readonly ZERO: Fp6; static readonly ONE: Fp6;
  readonly c0: Fp2; readonly c1: Fp2; readonly c2: Fp2;
  constructor(c0: Fp2, c1: Fp2, c2: Fp2);
  static fromBigSix(t: bigint[]): Fp6;
  one(): Fp6; isZero(): boolean; equals(rhs: Fp6): boolean; negate(): Fp6; add(rhs: Fp6): Fp6; subtract(rhs: Fp6): Fp6; multiply(rhs: Fp6 | bigint): Fp6;
  square(): Fp6; pow(n: bigint): Fp6; div(rhs: Fp6 | bigint): Fp6; invert(): Fp6; mulByNonresidue(): Fp6; frobeniusMap(power: number): Fp6; toString(): string;
  static fromBytes(b: Uint8Array): Fp6; toBytes(): Uint8Array;
}
export declare class Fp12 implements Field<Fp12> {
  static readonly BYTES_LEN: number; static readonly ZERO: Fp12; static readonly ONE: Fp12;
  readonly c0: Fp6; readonly c1: Fp6;
  constructor(c0: Fp6, c1: Fp6);
  static fromBigTwelve(t: bigint[]): Fp12;
  one(): Fp12; isZero(): boolean; equals(rhs: Fp12): boolean; negate(): Fp12; add(rhs: Fp12): Fp12; subtract(rhs: Fp12): Fp12; multiply(rhs: Fp12 | bigint): Fp12;
  square(): Fp12; pow(n: bigint): Fp12; div(rhs: Fp12 | bigint): Fp12; invert(): Fp12; conjugate(): Fp12; frobeniusMap(power: number): Fp12; toString(): string;
  /** runs on the GPU (nbls_final_exp_batch) */
  finalExponentiate(): Fp12;
  static fromBytes(b: Uint8Array): Fp12; toBytes(): Uint8Array;
  /** kilic / zkcrypto coefficient order (the twelve 48-byte words reversed; reference test/deterministic.test.ts:9-12, 41) */
  static fromKilicBytes(b: Uint8Array | string): Fp12; toKilicBytes(): Uint8Array;
}

export declare class PointG1 {
  static readonly BASE: PointG1; static readonly ZERO: PointG1;
  constructor(x: Fp, y: Fp, z?: Fp);
  readonly x: Fp; readonly y: Fp; readonly z: Fp;
  static fromHex(bytes: Hex): PointG1;
  static fromPrivateKey(privateKey: PrivateKey): PointG1;
  static hashToCurve(msg: Hex, options?: { DST?: string }): Promise<PointG1>;
  static encodeToCurve(msg: Hex, options?: { DST?: string }): Promise<PointG1>;
  /** additive: sum of points / multi-scalar multiplication on the GPU */
  static sum(points: PointG1[]): PointG1;
  static msm(points: PointG1[], scalars: (bigint | number)[]): PointG1;
  /** threshold recombination on the GPU: sum_k [lambda_k]share_k with the Lagrange coefficients at zero of the identifiers (any value below 2^256, reduced mod CURVE.r).
   *  Compressed shares (bytes or hex) give bytes, points give a point.  Throws Error on identifiers that are zero or repeated mod r and on a share that does not decode. */
  static combineShares(shares: PointG1[], ids: ShareId[]): Promise<PointG1>;
  static combineShares(shares: Hex[], ids: ShareId[]): Promise<Uint8Array>;
  static combineSharesBatch(groups: ShareGroup<PointG1>[]): Promise<(PointG1 | Uint8Array)[]>;
  /** share public keys on the GPU: the commitment polynomial F(x) = sum_j [x^j]A_j of a DKG / Feldman VSS (coefficients lowest degree first, A_0 = the group key) at the
   *  identifiers (any value below 2^256, zero included).  Compressed coefficients (bytes or hex) give bytes, points give points.  Throws Error on a coefficient that does not decode. */
  static evalCommitment(coefs: PointG1[], ids: ShareId[]): Promise<PointG1[]>;
  static evalCommitment(coefs: Hex[], ids: ShareId[]): Promise<Uint8Array[]>;
  static evalCommitmentBatch(groups: CommitmentGroup<PointG1>[]): Promise<(PointG1[] | Uint8Array[])[]>;
  /** EIP-4844 verify_kzg_proof_batch against the setup's [tau]G2; status: 0 ok, 9 not verified, 3 / 4 commitment, 13 / 14 proof, 21 non-canonical field element */
  static verifyKzgProofBatch(commitments: (PointG1 | Hex)[], zs: ShareId[], ys: ShareId[], proofs: (PointG1 | Hex)[], tauG2: PointG2 | Hex, opts?: KzgOptions): KzgResult;
  static verifyKzgProofBatchAsync(commitments: (PointG1 | Hex)[], zs: ShareId[], ys: ShareId[], proofs: (PointG1 | Hex)[], tauG2: PointG2 | Hex, opts?: KzgOptions): Promise<KzgResult>;
  /** EIP-4844 verify_blob_kzg_proof_batch: blobs of 32 * 2^k bytes (k = 12 on mainnet); the challenge is hashed on the host, the polynomial evaluated on the device */
  static verifyBlobKzgProofBatch(blobs: Hex[], commitments: (PointG1 | Hex)[], proofs: (PointG1 | Hex)[], tauG2: PointG2 | Hex, opts?: KzgOptions): KzgResult;
  static verifyBlobKzgProofBatchAsync(blobs: Hex[], commitments: (PointG1 | Hex)[], proofs: (PointG1 | Hex)[], tauG2: PointG2 | Hex, opts?: KzgOptions): Promise<KzgResult>;
  /** EIP-4844 blob_to_kzg_commitment / compute_kzg_proof / compute_blob_kzg_proof for many blobs; status: 0, or 21 (a non-canonical element: that blob's outputs are all-zero bytes) */
  static readonly KzgSetup: typeof KzgSetup;
  static blobToKzgCommitments(setup: KzgSetup, blobs: Hex[]): KzgCommitments;
  static blobToKzgCommitmentsAsync(setup: KzgSetup, blobs: Hex[]): Promise<KzgCommitments>;
  static computeKzgProofs(setup: KzgSetup, blobs: Hex[], zs: ShareId[]): KzgProofs;
  static computeKzgProofsAsync(setup: KzgSetup, blobs: Hex[], zs: ShareId[]): Promise<KzgProofs>;
  /** commitments given: only hashed into the challenge, not decoded; omitted: computed first and returned */
  static computeBlobKzgProofs(setup: KzgSetup, blobs: Hex[], commitments?: (PointG1 | Hex)[]): KzgBlobProofs;
  static computeBlobKzgProofsAsync(setup: KzgSetup, blobs: Hex[], commitments?: (PointG1 | Hex)[]): Promise<KzgBlobProofs>;
  /** PeerDAS (EIP-7594).  frNtt: n polynomials of 2^log2n elements; toEvals false: values on the roots (bit-reversed order) -> coefficients (natural order), true: the way back;
   *  shifts: one per polynomial (the values are those on shift * root), or omitted.  computeCells: 2^log2cell elements per cell (mainnet: log2n 12, log2cell 6) */
  static readonly KzgMonomialSetup: typeof KzgMonomialSetup;
  static frNtt(log2n: number, rows: Hex[], toEvals: boolean, shifts?: ShareId[]): FrNttRows;
  static frNttAsync(log2n: number, rows: Hex[], toEvals: boolean, shifts?: ShareId[]): Promise<FrNttRows>;
  static computeCells(log2n: number, log2cell: number, blobs: Hex[]): KzgCells;
  static computeCellsAsync(log2n: number, log2cell: number, blobs: Hex[]): Promise<KzgCells>;
  static computeCellsAndKzgProofs(setup: KzgMonomialSetup, log2cell: number, blobs: Hex[]): KzgCellsAndProofs;
  static computeCellsAndKzgProofsAsync(setup: KzgMonomialSetup, log2cell: number, blobs: Hex[]): Promise<KzgCellsAndProofs>;
  /** recover_cells_and_kzg_proofs (EIP-7594): cellIndices[i] = the numbers of the cells given for blob i (any order, at least half of them), cells[i] = those cells.  Results as
   *  computeCells / computeCellsAndKzgProofs return them for the recovered blobs; status per blob: 22 = fewer than half of the cells, an index out of range or twice,
   *  21 = an element >= CURVE.r, 23 = the given cells contradict one another (the blob's outputs are then all-zero bytes) */
  static recoverCells(log2n: number, log2cell: number, cellIndices: number[][], cells: Hex[][]): KzgCells;
  static recoverCellsAsync(log2n: number, log2cell: number, cellIndices: number[][], cells: Hex[][]): Promise<KzgCells>;
  static recoverCellsAndKzgProofs(setup: KzgMonomialSetup, log2cell: number, cellIndices: number[][], cells: Hex[][]): KzgCellsAndProofs;
  static recoverCellsAndKzgProofsAsync(setup: KzgMonomialSetup, log2cell: number, cellIndices: number[][], cells: Hex[][]): Promise<KzgCellsAndProofs>;
  /** EIP-7594 verify_cell_kzg_proof_batch: cell k is cell number cellIndices[k] of the blob with commitment commitments[commitmentIndices[k]] (every commitment once; cells of
   *  32 << log2cell bytes, log2cell <= 6) against the setup's [tau^c]G2; status as verifyKzgProofBatch, 21 = an element of the cell is non-canonical */
  static verifyCellKzgProofBatch(setup: KzgMonomialSetup, log2cell: number, commitments: (PointG1 | Hex)[], commitmentIndices: number[], cellIndices: number[], cells: Hex[],
    proofs: (PointG1 | Hex)[], tauCG2: PointG2 | Hex, opts?: KzgOptions): KzgResult;
  static verifyCellKzgProofBatchAsync(setup: KzgMonomialSetup, log2cell: number, commitments: (PointG1 | Hex)[], commitmentIndices: number[], cellIndices: number[], cells: Hex[],
    proofs: (PointG1 | Hex)[], tauCG2: PointG2 | Hex, opts?: KzgOptions): Promise<KzgResult>;
  /** Groth16 over BLS12-381: n proofs (192 bytes each, A || B || C compressed; an array of bytes / hex or ONE packed Uint8Array) with their rows of public inputs (an array of
   *  rows, or ONE packed Uint8Array of 32 bytes per input) against one key, by a random linear combination; status per proof: 0, 9 not verified, 1 / 3 / 4 A, 11 / 13 / 14 B,
   *  31 / 33 / 34 C (the zero point / does not decode), 21 a non-canonical input */
  static readonly Groth16Vk: typeof Groth16Vk;
  static verifyGroth16Batch(vk: Groth16Vk, proofs: Hex[] | Uint8Array, inputs: ShareId[][] | Uint8Array, opts?: KzgOptions): KzgResult;
  static verifyGroth16BatchAsync(vk: Groth16Vk, proofs: Hex[] | Uint8Array, inputs: ShareId[][] | Uint8Array, opts?: KzgOptions): Promise<KzgResult>;
  /** The Groth16 prover: one proof (192 bytes, A || B || C compressed) per witness z = [1, x_1 .. x_m, aux ..] against a proving key on the device; rs: [r, s] per witness, or
   *  null: drawn from the OS.  status per proof: 0, 21 an element >= CURVE.r, 24 the witness does not satisfy the constraints, 1 A or B is the zero point (192 zero bytes then) */
  static readonly Groth16Pk: typeof Groth16Pk;
  static groth16ProvingKey(key: Groth16PkInit): Groth16Pk;
  static groth16Prove(pk: Groth16Pk, witnesses: ShareId[][] | Uint8Array, rs?: [ShareId, ShareId][] | null): { proofs: Uint8Array[]; status: Uint8Array };
  isZero(): boolean; equals(rhs: PointG1): boolean; negate(): PointG1; add(rhs: PointG1): PointG1; subtract(rhs: PointG1): PointG1; double(): PointG1;
  multiply(scalar: bigint | number): PointG1; multiplyUnsafe(scalar: bigint | number): PointG1; multiplyPrecomputed(scalar: bigint | number): PointG1;
  assertValidity(): this; toAffine(): [Fp, Fp]; toRawBytes(isCompressed?: boolean): Uint8Array; toHex(isCompressed?: boolean): string;
  millerLoop(P: PointG2): Fp12; clearCofactor(): PointG1; toString(): string;
}
export declare class PointG2 {
  static readonly BASE: PointG2; static readonly ZERO: PointG2;
  constructor(x: Fp2, y: Fp2, z?: Fp2);
  readonly x: Fp2; readonly y: Fp2; readonly z: Fp2;
  static fromHex(bytes: Hex): PointG2;
  static fromSignature(hex: Hex): PointG2;
  static fromPrivateKey(privateKey: PrivateKey): PointG2;
  static hashToCurve(msg: Hex, options?: { DST?: string }): Promise<PointG2>;
  static encodeToCurve(msg: Hex, options?: { DST?: string }): Promise<PointG2>;
  static sum(points: PointG2[]): PointG2;
  static msm(points: PointG2[], scalars: (bigint | number)[]): PointG2;
  /** threshold recombination on the GPU: sum_k [lambda_k]share_k with the Lagrange coefficients at zero of the identifiers (any value below 2^256, reduced mod CURVE.r).
   *  Compressed shares (bytes or hex) give bytes, points give a point.  Throws Error on identifiers that are zero or repeated mod r and on a share that does not decode. */
  static combineShares(shares: PointG2[], ids: ShareId[]): Promise<PointG2>;
  static combineShares(shares: Hex[], ids: ShareId[]): Promise<Uint8Array>;
  static combineSharesBatch(groups: ShareGroup<PointG2>[]): Promise<(PointG2 | Uint8Array)[]>;
  /** share public keys on the GPU: the commitment polynomial F(x) = sum_j [x^j]A_j of a DKG / Feldman VSS (coefficients lowest degree first, A_0 = the group key) at the
   *  identifiers (any value below 2^256, zero included).  Compressed coefficients (bytes or hex) give bytes, points give points.  Throws Error on a coefficient that does not decode. */
  static evalCommitment(coefs: PointG2[], ids: ShareId[]): Promise<PointG2[]>;
  static evalCommitment(coefs: Hex[], ids: ShareId[]): Promise<Uint8Array[]>;
  static evalCommitmentBatch(groups: CommitmentGroup<PointG2>[]): Promise<(PointG2[] | Uint8Array[])[]>;
  isZero(): boolean; equals(rhs: PointG2): boolean; negate(): PointG2; add(rhs: PointG2): PointG2; subtract(rhs: PointG2): PointG2; double(): PointG2;
  multiply(scalar: bigint | number): PointG2; multiplyUnsafe(scalar: bigint | number): PointG2; multiplyPrecomputed(scalar: bigint | number): PointG2;
  assertValidity(): this; toAffine(): [Fp2, Fp2]; toSignature(): Uint8Array; toRawBytes(isCompressed?: boolean): Uint8Array; toHex(isCompressed?: boolean): string;
  toString(): string;
}

export declare function pairing(P: PointG1, Q: PointG2, withFinalExponent?: boolean): Fp12;
export declare function getPublicKey(privateKey: PrivateKey): Uint8Array;
export declare function sign(message: Hex, privateKey: PrivateKey): Promise<Uint8Array>;
export declare function sign(message: PointG2, privateKey: PrivateKey): Promise<PointG2>;
export declare function verify(signature: Hex | PointG2, message: Hex | PointG2, publicKey: Hex | PointG1): Promise<boolean>;
export declare function aggregatePublicKeys(publicKeys: Hex[]): Uint8Array;
export declare function aggregatePublicKeys(publicKeys: PointG1[]): PointG1;
export declare function aggregateSignatures(signatures: Hex[]): Uint8Array;
export declare function aggregateSignatures(signatures: PointG2[]): PointG2;
export declare function verifyBatch(signature: Hex | PointG2, messages: (Hex | PointG2)[], publicKeys: (Hex | PointG1)[]): Promise<boolean>;
/** verify(signature, message, publicKey) for every set, checked together by a random linear combination on the GPU; throws where verify throws for the first such set */
export declare function verifyMultipleSignatures(sets: { publicKey: Hex | PointG1; message: Hex | PointG2; signature: Hex | PointG2 }[]): Promise<boolean>;
/** verify(signature, message, aggregatePublicKeys(publicKeys)) for every set, checked together by a random linear combination on the GPU; throws where that throws for the first such set */
export declare function verifyMultipleAggregateSignatures(sets: { publicKeys: (Hex | PointG1)[]; message: Hex | PointG2; signature: Hex | PointG2 }[]): Promise<boolean>;
export type ShareId = bigint | number | string | Uint8Array;
/** KZG: seed = 32 bytes for reproducible weights (default: from the OS); perItem === false stops after the combined check (status null) */
export interface KzgOptions { seed?: Hex; perItem?: boolean }
/** A trusted setup's g1_lagrange (2^k points in bit-reversed order, 1 <= k <= 12) decoded once into device memory; close() frees it.  Reached as PointG1.KzgSetup */
declare class KzgSetup {
  constructor(points: (PointG1 | Hex)[]);
  readonly log2n: number;
  close(): void;
}
/** A trusted setup's g1_monomial (2^k points [tau^i]G1 in natural order, 1 <= k <= 12) decoded once into device memory; close() frees it.  Reached as PointG1.KzgMonomialSetup */
declare class KzgMonomialSetup {
  constructor(points: (PointG1 | Hex)[]);
  readonly log2n: number;
  close(): void;
}
/** A Groth16 verifying key decoded once into device memory (alpha and the m + 1 points ic in G1, beta, gamma, delta in G2, all compressed); close() frees it.  Parsing
 *  bellman's uncompressed key file stays with the caller.  Reached as PointG1.Groth16Vk */
declare class Groth16Vk {
  constructor(key: { alpha: PointG1 | Hex; beta: PointG2 | Hex; gamma: PointG2 | Hex; delta: PointG2 | Hex; ic: (PointG1 | Hex)[] });
  readonly inputs: number;
  close(): void;
}
/** An R1CS instance and its Groth16 proving key: a matrix is an array of rows (at most 2^log2n, the same number in all three), a row an array of [column, coefficient];
 *  the queries hold nVars, nVars, nVars, nVars - nPublic - 1 and 2^log2n - 1 compressed points; a zero point is valid in the four per-variable queries */
export interface Groth16PkInit {
  log2n: number; nVars: number; nPublic: number; matrices: [number, ShareId][][][];
  alphaG1: PointG1 | Hex; betaG1: PointG1 | Hex; betaG2: PointG2 | Hex; deltaG1: PointG1 | Hex; deltaG2: PointG2 | Hex;
  aQuery: (PointG1 | Hex)[]; bG1Query: (PointG1 | Hex)[]; bG2Query: (PointG2 | Hex)[]; lQuery: (PointG1 | Hex)[]; hQuery: (PointG1 | Hex)[];
}
/** A Groth16 proving key decoded once into device memory with the workspace of a proof; close() frees it.  Reading bellman's or snarkjs's key files stays with the caller.
 *  Reached as PointG1.Groth16Pk / PointG1.groth16ProvingKey */
declare class Groth16Pk {
  constructor(key: Groth16PkInit);
  readonly log2n: number; readonly nVars: number; readonly nPublic: number;
  close(): void;
}
/** status: one byte per polynomial (0; 21 an element or the shift is >= CURVE.r; 5 the shift is 0: the row is then all-zero) */
export interface FrNttRows { rows: Uint8Array[]; status: Uint8Array }
/** cells[blob][k]: the 32 << log2cell bytes of cell k; proofs[blob][k]: its 48-byte proof; status: one byte per blob (21: an element >= CURVE.r, cells all-zero, proofs 48 zero bytes) */
export interface KzgCells { cells: Uint8Array[][]; status: Uint8Array }
export interface KzgCellsAndProofs { cells: Uint8Array[][]; proofs: Uint8Array[][]; status: Uint8Array }
export interface KzgCommitments { commitments: Uint8Array[]; status: Uint8Array }
export interface KzgProofs { proofs: Uint8Array[]; ys: Uint8Array[]; status: Uint8Array }
export interface KzgBlobProofs { commitments: Uint8Array[]; proofs: Uint8Array[]; status: Uint8Array }
export interface KzgResult { ok: boolean; status: Uint8Array | null }
/** one group of combineSharesBatch: its shares are all points or all compressed bytes / hex */
export type ShareGroup<P> = { shares: P[] | Hex[]; ids: ShareId[] } | [P[] | Hex[], ShareId[]];
/** one group of evalCommitmentBatch: its coefficients are all points or all compressed bytes / hex */
export type CommitmentGroup<P> = { coefs: P[] | Hex[]; ids: ShareId[] } | [P[] | Hex[], ShareId[]];
/** what the addon's Fr and threshold calls take (nbls_fr_op_batch, nbls_lagrange_at_zero, nbls_g2_combine_shares / nbls_g1_combine_shares; a type only, the facade does not export
 * the addon): 32-byte big-endian elements, groupOffsets = groups + 1 entries; every call has a synchronous twin without the suffix */
export interface NativeThresholdCalls {
  frOpAsync(op: number, a32: Uint8Array, b32: Uint8Array | null): Promise<{ out: Uint8Array; status: Uint8Array }>;
  lagrangeAtZeroAsync(groupOffsets: Uint32Array, ids32: Uint8Array): Promise<{ out: Uint8Array; status: Uint8Array }>;
  combineSharesAsync(g2: number, groupOffsets: Uint32Array, ids32: Uint8Array, shares: Uint8Array): Promise<{ out: Uint8Array; status: Uint8Array }>;
  /** nbls_g1_poly_eval / nbls_g2_poly_eval: one compressed point and one status per identifier */
  polyEvalAsync(g2: number, coefOffsets: Uint32Array, coefs: Uint8Array, idOffsets: Uint32Array, ids32: Uint8Array): Promise<{ out: Uint8Array; status: Uint8Array }>;
  /** nbls_kzg_verify_proofs / nbls_kzg_verify_blobs: out = the verdict as a native int (4 bytes), status = one byte per item */
  kzgVerifyProofs(commitments48: Uint8Array, z32: Uint8Array, y32: Uint8Array, proofs48: Uint8Array, tauG2: Uint8Array, seed32: Uint8Array | null, perItem: number): { out: Uint8Array; status: Uint8Array };
  kzgVerifyProofsAsync(commitments48: Uint8Array, z32: Uint8Array, y32: Uint8Array, proofs48: Uint8Array, tauG2: Uint8Array, seed32: Uint8Array | null, perItem: number): Promise<{ out: Uint8Array; status: Uint8Array }>;
  kzgVerifyBlobs(log2n: number, blobs: Uint8Array, commitments48: Uint8Array, proofs48: Uint8Array, tauG2: Uint8Array, seed32: Uint8Array | null, perItem: number): { out: Uint8Array; status: Uint8Array };
  kzgVerifyBlobsAsync(log2n: number, blobs: Uint8Array, commitments48: Uint8Array, proofs48: Uint8Array, tauG2: Uint8Array, seed32: Uint8Array | null, perItem: number): Promise<{ out: Uint8Array; status: Uint8Array }>;
  /** nbls_kzg_setup_create / _destroy and the three prover calls (kind 0 commitments, 1 proofs at aux = z32, 2 blob proofs with aux = commitments48 or null); out = two arrays of n entries one behind the other */
  kzgSetupCreate(log2n: number, lagrange48: Uint8Array): unknown;
  kzgSetupDestroy(handle: unknown): void;
  kzgProve(kind: number, handle: unknown, blobs: Uint8Array, aux: Uint8Array | null): { out: Uint8Array; status: Uint8Array };
  kzgProveAsync(kind: number, handle: unknown, blobs: Uint8Array, aux: Uint8Array | null): Promise<{ out: Uint8Array; status: Uint8Array }>;
}
/** The two calls of the N-API addon (nbls_napi.node) that verifyMultipleSignatures / verifyMultipleAggregateSignatures take when at least two wire-format sets have equal messages:
 * msgs / offsets hold the distinct messages, set i signs message msgIndex[i] (nbls_verify_multiple_shared / nbls_verify_aggregates_shared; a type only, the facade does not export the addon) */
export interface NativeSharedCalls {
  verifyMultipleSharedAsync(sigs96: Uint8Array, msgs: Uint8Array, offsets: Uint32Array, msgIndex: Uint32Array, pks48: Uint8Array, dst: Uint8Array): Promise<{ ok: boolean; status: Uint8Array }>;
  verifyAggregatesSharedAsync(sigs96: Uint8Array, msgs: Uint8Array, offsets: Uint32Array, msgIndex: Uint32Array, pks48: Uint8Array, keyOffsets: Uint32Array, dst: Uint8Array): Promise<{ ok: boolean; status: Uint8Array }>;
}

// additive batched entry points (one engine call each)
export declare function pairingBatch(Ps: PointG1[] | Uint8Array /* n x 96 affine bytes */, Qs: PointG2[] | Uint8Array /* n x 192 */, withFinalExponent?: boolean, validate?: boolean): { out: Uint8Array /* n x 576 */; status: Uint8Array };
export declare function millerProduct(Ps: PointG1[] | Uint8Array, Qs: PointG2[] | Uint8Array, finalExponent?: boolean, validate?: boolean): { out: Uint8Array /* 576 */; status: Uint8Array };
export declare function getPublicKeys(privateKeys: PrivateKey[]): Uint8Array[];
export declare function signBatch(messages: Hex[], privateKeys: PrivateKey[]): Promise<Uint8Array[]>;
/** contexts (1..8, default NBLS_CONTEXTS or 1): engine contexts that asynchronous verifyBatch calls take round-robin, so that concurrent promises overlap on the GPU */
export declare function init(deviceId?: number, contexts?: number): void;

export declare const utils: {
  hashToField(msg: Uint8Array, count: number, options?: { DST?: string; p?: bigint; m?: number; k?: number; expand?: boolean; hash?: (m: Uint8Array) => Promise<Uint8Array> }): Promise<bigint[][]>;
  expandMessageXMD(msg: Uint8Array, DST: Uint8Array, lenInBytes: number, H?: (m: Uint8Array) => Promise<Uint8Array>): Promise<Uint8Array>;
  hashToPrivateKey(hash: Hex): Uint8Array;
  stringToBytes(str: string): Uint8Array; bytesToHex(b: Uint8Array): string; hexToBytes(hex: string): Uint8Array;
  randomBytes(bytesLength?: number): Uint8Array; randomPrivateKey(): Uint8Array;
  sha256(message: Uint8Array): Promise<Uint8Array>; mod(a: bigint, b: bigint): bigint;
  getDSTLabel(): string; setDSTLabel(newLabel: string): void;
};
